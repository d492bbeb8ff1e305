// pch.h -- TEST INFRASTRUCTURE ONLY.
//
// Stand-in for the reference's precompiled header, written from scratch for `make -C oracle ref`: it lets the
// reference's geometry units (Src/Poly.cpp, Src/Kdop.cpp, Src/VMACH.cpp) compile with g++ on Linux, with no Windows,
// COM, D3D12 or DirectXMath header.  It sits ahead of the reference's Inc/ on the include path.  Nothing in it is taken
// from the reference tree or from DirectXMath / SimpleMath: only the names the three units use are declared, and every
// operation is written out in scalar float32.
//
// ARITHMETIC.  The reference runs SimpleMath over DirectXMath's SSE2 path on x64 (no /arch:AVX2, so no fused
// multiply-add and no dpps).  SSE lanes are independent IEEE-754 float32 operations, so each lane-wise intrinsic equals
// the scalar float32 expression below, provided the compiler neither contracts a*b+c nor reassociates: build with
// -ffp-contract=off -fno-fast-math.  Each operation carries a one-line reason for the form chosen.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <exception>
#include <iterator>
#include <limits>
#include <list>
#include <map>
#include <memory>
#include <numeric>
#include <queue>
#include <random>
#include <set>
#include <stdexcept>
#include <string>
#include <tuple>
#include <unordered_map>
#include <unordered_set>
#include <vector>

constexpr double EPSILON = 1.0e-12;      // the geometric epsilon the units compare lengths with: a setting, stated as a number

// The few Win32 spellings the geometry units use.
#ifndef TRUE
#define TRUE 1
#endif
#ifndef FALSE
#define FALSE 0
#endif
#define _In_
#define _Out_
#define _Inout_

namespace DirectX
{

constexpr float XM_2PI = 6.283185307f;      // 2*pi rounded to float32, as DirectXMath publishes it

struct XMFLOAT3
{
    float x, y, z;
    XMFLOAT3() : x(0.f), y(0.f), z(0.f) {}
    XMFLOAT3(float ix, float iy, float iz) : x(ix), y(iy), z(iz) {}
};

struct XMFLOAT4
{
    float x, y, z, w;
    XMFLOAT4() : x(0.f), y(0.f), z(0.f), w(0.f) {}
    XMFLOAT4(float ix, float iy, float iz, float iw) : x(ix), y(iy), z(iz), w(iw) {}
};

// A four-lane register.  Loading a float3 leaves w = 0 (XMLoadFloat3).
struct XMVECTOR
{
    float x, y, z, w;
};
typedef const XMVECTOR& FXMVECTOR;

// Four row registers.
struct XMMATRIX
{
    XMVECTOR r[4];
    XMMATRIX() : r{} {}
    XMMATRIX(float m00, float m01, float m02, float m03, float m10, float m11, float m12, float m13,
             float m20, float m21, float m22, float m23, float m30, float m31, float m32, float m33)
        : r{{m00, m01, m02, m03}, {m10, m11, m12, m13}, {m20, m21, m22, m23}, {m30, m31, m32, m33}}
    {
    }
};
typedef const XMMATRIX& FXMMATRIX;

// XMMatrixTranspose: a shuffle, no arithmetic.
inline XMMATRIX XMMatrixTranspose(FXMMATRIX m)
{
    XMMATRIX t;
    t.r[0] = {m.r[0].x, m.r[1].x, m.r[2].x, m.r[3].x};
    t.r[1] = {m.r[0].y, m.r[1].y, m.r[2].y, m.r[3].y};
    t.r[2] = {m.r[0].z, m.r[1].z, m.r[2].z, m.r[3].z};
    t.r[3] = {m.r[0].w, m.r[1].w, m.r[2].w, m.r[3].w};
    return t;
}

// XMVector3TransformCoord: three multiply-adds starting from row 3 (z first, then y, then x), each a separate multiply
// and add without FMA, then a lane-wise divide by the w lane: x*m0 + (y*m1 + (z*m2 + m3)), result / result.w.
inline XMVECTOR XMVector3TransformCoord(FXMVECTOR v, FXMMATRIX m)
{
    float o[4];
    const float* r0 = &m.r[0].x;
    const float* r1 = &m.r[1].x;
    const float* r2 = &m.r[2].x;
    const float* r3 = &m.r[3].x;
    for (int c = 0; c < 4; ++c)
    {
        float t = v.z * r2[c];
        t = t + r3[c];
        float u = v.y * r1[c];
        t = u + t;
        float w = v.x * r0[c];
        o[c] = w + t;
    }
    return XMVECTOR{o[0] / o[3], o[1] / o[3], o[2] / o[3], o[3] / o[3]};
}

namespace SimpleMath
{

struct Vector3 : public XMFLOAT3
{
    Vector3() : XMFLOAT3(0.f, 0.f, 0.f) {}
    explicit Vector3(float s) : XMFLOAT3(s, s, s) {}
    Vector3(float ix, float iy, float iz) : XMFLOAT3(ix, iy, iz) {}      // double arguments narrow to float32 here
    Vector3(const XMFLOAT3& f) : XMFLOAT3(f.x, f.y, f.z) {}
    Vector3(FXMVECTOR v) : XMFLOAT3(v.x, v.y, v.z) {}                    // a store of three lanes

    operator XMVECTOR() const { return XMVECTOR{x, y, z, 0.f}; }         // a load of three lanes, w = 0

    // XMVector3Equal / NotEqual: lane-wise compare of x, y, z.
    bool operator==(const Vector3& v) const { return x == v.x && y == v.y && z == v.z; }
    bool operator!=(const Vector3& v) const { return !(x == v.x && y == v.y && z == v.z); }

    // XMVectorAdd / Subtract / Multiply: one float32 operation per lane.
    Vector3& operator+=(const Vector3& v) { x = x + v.x; y = y + v.y; z = z + v.z; return *this; }
    Vector3& operator-=(const Vector3& v) { x = x - v.x; y = y - v.y; z = z - v.z; return *this; }
    Vector3& operator*=(const Vector3& v) { x = x * v.x; y = y * v.y; z = z * v.z; return *this; }
    // XMVectorScale: the scalar is splatted, then one multiply per lane.
    Vector3& operator*=(float s) { x = x * s; y = y * s; z = z * s; return *this; }
    // SimpleMath divides a vector by a scalar as a scale by the float32 reciprocal 1.f / S, not as a division.
    Vector3& operator/=(float s) { const float r = 1.f / s; x = x * r; y = y * r; z = z * r; return *this; }
    // XMVectorNegate on SSE is 0 - v per lane (so the negative of +0 is +0).
    Vector3 operator-() const { return Vector3(0.f - x, 0.f - y, 0.f - z); }

    // XMVector3Dot on SSE2: lane products, then (x + y) + z with scalar adds.
    float Dot(const Vector3& v) const
    {
        const float px = x * v.x, py = y * v.y, pz = z * v.z;
        const float t = px + py;
        return t + pz;
    }
    // XMVector3Cross: (y*z' - z*y', z*x' - x*z', x*y' - y*x'), each product rounded before the subtraction (no FMA).
    Vector3 Cross(const Vector3& v) const
    {
        const float a = y * v.z, b = z * v.y;
        const float c = z * v.x, d = x * v.z;
        const float e = x * v.y, f = y * v.x;
        return Vector3(a - b, c - d, e - f);
    }
    // XMVector3LengthSq is the dot with itself; XMVector3Length takes sqrtps of it (correctly rounded).
    float LengthSquared() const { return Dot(*this); }
    float Length() const { return std::sqrt(Dot(*this)); }
    // XMVector3Normalize on SSE2: divide every lane by sqrt(dot); a zero length gives the zero vector, an infinite
    // length a quiet NaN.  A division, not a multiplication by a reciprocal.
    void Normalize()
    {
        const float l2 = Dot(*this);
        const float l = std::sqrt(l2);
        if (l2 == 0.f) { x = y = z = 0.f; return; }
        if (l2 == std::numeric_limits<float>::infinity())
        {
            x = y = z = std::numeric_limits<float>::quiet_NaN();
            return;
        }
        x = x / l; y = y / l; z = z / l;
    }
};

// Binary operators: the same lane-wise operations as the compound forms above.
inline Vector3 operator+(const Vector3& a, const Vector3& b) { return Vector3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline Vector3 operator-(const Vector3& a, const Vector3& b) { return Vector3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline Vector3 operator*(const Vector3& a, const Vector3& b) { return Vector3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline Vector3 operator*(const Vector3& a, float s) { return Vector3(a.x * s, a.y * s, a.z * s); }
inline Vector3 operator*(float s, const Vector3& a) { return Vector3(a.x * s, a.y * s, a.z * s); }
// XMVectorDivide: one divide per lane.
inline Vector3 operator/(const Vector3& a, const Vector3& b) { return Vector3(a.x / b.x, a.y / b.y, a.z / b.z); }
// Vector / scalar: scale by the float32 reciprocal, as operator/= above.
inline Vector3 operator/(const Vector3& a, float s) { const float r = 1.f / s; return Vector3(a.x * r, a.y * r, a.z * r); }

struct Plane : public XMFLOAT4
{
    Plane() : XMFLOAT4(0.f, 1.f, 0.f, 0.f) {}
    Plane(float ix, float iy, float iz, float iw) : XMFLOAT4(ix, iy, iz, iw) {}
    Plane(const Vector3& normal, float d) : XMFLOAT4(normal.x, normal.y, normal.z, d) {}
    // XMPlaneFromPointNormal: the normal is kept as given (not normalised), w = 0 - dot(point, normal).
    Plane(const Vector3& point, const Vector3& normal) : XMFLOAT4(normal.x, normal.y, normal.z, 0.f - point.Dot(normal)) {}
    // XMPlaneFromPoints: n = normalize(cross(p1 - p2, p1 - p3)), w = 0 - dot(n, p1).
    Plane(const Vector3& p1, const Vector3& p2, const Vector3& p3)
    {
        Vector3 n = (p1 - p2).Cross(p1 - p3);
        n.Normalize();
        x = n.x; y = n.y; z = n.z;
        w = 0.f - n.Dot(p1);
    }

    bool operator==(const Plane& p) const { return x == p.x && y == p.y && z == p.z && w == p.w; }
    bool operator!=(const Plane& p) const { return !(*this == p); }

    Vector3 Normal() const { return Vector3(x, y, z); }
    void Normal(const Vector3& n) { x = n.x; y = n.y; z = n.z; }
    float D() const { return w; }
    void D(float d) { w = d; }

    // XMPlaneNormalize on SSE2: all four lanes divided by sqrt(dot3(normal)); an infinite length gives zero.
    void Normalize()
    {
        const float l2 = Normal().Dot(Normal());
        const float l = std::sqrt(l2);
        if (l2 == std::numeric_limits<float>::infinity()) { x = y = z = w = 0.f; return; }
        x = x / l; y = y / l; z = z / l; w = w / l;
    }
    // XMPlaneDotCoord / XMPlaneDotNormal: ((x*x' + y*y') + z*z') + w, and the three-lane dot.
    float DotCoordinate(const Vector3& p) const { return Normal().Dot(p) + w; }
    float DotNormal(const Vector3& n) const { return Normal().Dot(n); }
};

} // namespace SimpleMath
} // namespace DirectX

// The reference's units name these without qualification.
using DirectX::XMFLOAT3;
using DirectX::XMMATRIX;
using DirectX::XMVECTOR;
using DirectX::XM_2PI;

// Inc/Mesh.h declares the vertex format beside D3D12 resources.  Only the vertex format is geometry: three float3
// (position, normal, colour).  Defining its include guard keeps the D3D12 half out.
#define MESH_H
struct VertexNormalColor
{
    DirectX::XMFLOAT3 Position;
    DirectX::XMFLOAT3 Normal;
    DirectX::XMFLOAT3 Color;
    explicit VertexNormalColor(const DirectX::XMFLOAT3& p = DirectX::XMFLOAT3(0.f, 0.f, 0.f),
                               const DirectX::XMFLOAT3& n = DirectX::XMFLOAT3(0.f, 0.f, 0.f),
                               const DirectX::XMFLOAT3& c = DirectX::XMFLOAT3(0.25f, 0.25f, 0.25f))
        : Position(p), Normal(n), Color(c)
    {
    }
};

// Helpers the reference keeps in its own pch.h; equivalents of ours with the same behaviour.

// Appends to `out` every element of `in` that `out` does not hold yet: first occurrences, in order.
template <typename T> static void UniqueVector(const std::vector<T>& in, std::vector<T>& out)
{
    for (const T& e : in)
    {
        bool seen = false;
        for (const T& o : out)
            if (o == e) { seen = true; break; }
        if (!seen) out.push_back(e);
    }
}

// Debug output goes nowhere.
#define OutputDebugStringWFormat(...) ((void)0)
#define OutputDebugStringW(...) ((void)0)
