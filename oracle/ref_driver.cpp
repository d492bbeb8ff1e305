// ref_driver.cpp -- TEST INFRASTRUCTURE ONLY.
//
// Runs one batch of cases through the reference's own geometry code, compiled by `make -C oracle ref` from the reference
// tree with the stand-in headers of oracle/ref_shim, and writes what it returned.  oracle/ref_compiled.py writes the
// batch and reads the results; tests/test_reference_compiled.py compares them with the oracle.
//
//   ref_driver <batch file> <result file>
//
// Both files are streams of 4-byte little-endian words (int32 / uint32 / float32; a double takes two words).
//   batch :  n_cases, then per case: op, payload
//   result:  per case: op, status (0 = returned, 2 = the reference threw), payload
// A solid travels as nv, pos[3 nv], off[nv + 1], nbr[off[nv]].  The result file is flushed after every case, so when the
// reference indexes outside a vector (-D_GLIBCXX_ASSERTIONS aborts there) the cases before it are complete and the
// first missing one is the one that aborted.
#include "pch.h"

#include "Poly.h"
#include "Kdop.h"
#include "VMACH.h"

#include <cstdio>

using DirectX::SimpleMath::Plane;
using DirectX::SimpleMath::Vector3;

namespace
{

enum Op { CLIP = 1, FACES = 2, RENDER = 3, NEIGHBOURS = 4, MOMENTS = 5, TRANSFORM = 6, KDOP = 7, REFIT = 8, HULL = 9 };

struct In
{
    std::vector<uint32_t> w;
    size_t at = 0;
    uint32_t u() { if (at >= w.size()) { std::fprintf(stderr, "batch file ends early\n"); std::exit(3); } return w[at++]; }
    int32_t i() { uint32_t v = u(); int32_t r; std::memcpy(&r, &v, 4); return r; }
    float f() { uint32_t v = u(); float r; std::memcpy(&r, &v, 4); return r; }
    double d() { uint32_t v[2] = {u(), u()}; double r; std::memcpy(&r, v, 8); return r; }
};

struct Out
{
    FILE* fp = nullptr;
    void u(uint32_t v) { std::fwrite(&v, 4, 1, fp); }
    void i(int32_t v) { std::fwrite(&v, 4, 1, fp); }
    void f(float v) { std::fwrite(&v, 4, 1, fp); }
    void d(double v) { std::fwrite(&v, 8, 1, fp); }
};

Poly::Polyhedron solid_in(In& in)
{
    const uint32_t nv = in.u();
    std::vector<Vector3> pos(nv);
    for (uint32_t v = 0; v < nv; ++v) { float x = in.f(), y = in.f(), z = in.f(); pos[v] = Vector3(x, y, z); }
    std::vector<uint32_t> off(nv + 1);
    for (uint32_t v = 0; v <= nv; ++v) off[v] = in.u();
    std::vector<std::vector<int>> nbr(nv);
    for (uint32_t v = 0; v < nv; ++v)
        for (uint32_t k = off[v]; k < off[v + 1]; ++k) nbr[v].push_back(in.i());
    Poly::Polyhedron p;
    Poly::InitPolyhedron(p, pos, nbr);
    return p;
}

void solid_out(Out& out, const Poly::Polyhedron& p)
{
    out.u((uint32_t)p.size());
    for (const Poly::Vertex& v : p) { out.f(v.Position.x); out.f(v.Position.y); out.f(v.Position.z); }
    uint32_t o = 0;
    out.u(o);
    for (const Poly::Vertex& v : p) { o += (uint32_t)v.NeighborVertexVec.size(); out.u(o); }
    for (const Poly::Vertex& v : p)
        for (int a : v.NeighborVertexVec) out.i(a);
}

std::vector<Vector3> points_in(In& in)
{
    const uint32_t n = in.u();
    std::vector<Vector3> p(n);
    for (uint32_t v = 0; v < n; ++v) { float x = in.f(), y = in.f(), z = in.f(); p[v] = Vector3(x, y, z); }
    return p;
}

// The face normals of the limited hull, taken from the hull's faces exactly as the reference's event loop takes them
// before it hands them to Kdop::KdopContainer: cross of the two edges from vertex 0, normalised.
std::vector<Vector3> hull_normals(const std::vector<Vector3>& pts, int limit)
{
    VMACH::ConvexHull hull(pts, (uint32_t)limit);
    std::vector<Vector3> out;
    for (const VMACH::ConvexHullFace& f : hull.GetFaces())
    {
        Vector3 n = (f.Vertices[1] - f.Vertices[0]).Cross(f.Vertices[2] - f.Vertices[0]);
        n.Normalize();
        out.push_back(n);
    }
    return out;
}

void run_case(In& in, Out& out)
{
    const int op = in.i();
    switch (op)
    {
    case CLIP:
    {
        Poly::Polyhedron p = solid_in(in);
        const uint32_t np = in.u();
        std::vector<Plane> planes(np);
        for (uint32_t k = 0; k < np; ++k) { float x = in.f(), y = in.f(), z = in.f(), w = in.f(); planes[k] = Plane(x, y, z, w); }
        Poly::ClipPolyhedron(p, planes);
        out.i(op); out.i(0); solid_out(out, p);
        break;
    }
    case FACES:
    {
        Poly::Polyhedron p = solid_in(in);
        std::unique_ptr<Poly::Extract> faces(Poly::ExtractFaces(p));
        out.i(op); out.i(0);
        out.u((uint32_t)faces->size());
        for (const auto& f : *faces) out.u((uint32_t)f.size());
        for (const auto& f : *faces)
            for (int v : f) out.i(v);
        break;
    }
    case RENDER:
    {
        Poly::Polyhedron p = solid_in(in);
        const int convex = in.i();
        float r = in.f(), g = in.f(), b = in.f();
        std::unique_ptr<Poly::Extract> faces(Poly::ExtractFaces(p));
        std::vector<VertexNormalColor> vd;
        std::vector<uint32_t> id;
        Poly::RenderPolyhedron(vd, id, p, faces.get(), convex != 0, Vector3(r, g, b));
        out.i(op); out.i(0);
        out.u((uint32_t)vd.size());
        for (const VertexNormalColor& v : vd)
        {
            out.f(v.Position.x); out.f(v.Position.y); out.f(v.Position.z);
            out.f(v.Normal.x); out.f(v.Normal.y); out.f(v.Normal.z);
            out.f(v.Color.x); out.f(v.Color.y); out.f(v.Color.z);
        }
        out.u((uint32_t)id.size());
        for (uint32_t v : id) out.u(v);
        break;
    }
    case NEIGHBOURS:
    {
        std::vector<Vector3> pos = points_in(in);
        const uint32_t ni = in.u();
        std::vector<int> idx(ni);
        for (uint32_t k = 0; k < ni; ++k) idx[k] = in.i();
        std::vector<std::vector<int>> rings;
        int status = 0;
        try { rings = Poly::ExtractNeighborFromMesh(pos, idx); }
        catch (const std::exception&) { status = 2; }
        out.i(op); out.i(status);
        if (status == 0)
        {
            out.u((uint32_t)rings.size());
            for (const auto& r : rings) out.u((uint32_t)r.size());
            for (const auto& r : rings)
                for (int v : r) out.i(v);
        }
        break;
    }
    case MOMENTS:
    {
        Poly::Polyhedron p = solid_in(in);
        double vol = 0.0;
        Vector3 first;
        Poly::Moments(vol, first, p);
        out.i(op); out.i(0);
        out.d(vol); out.f(first.x); out.f(first.y); out.f(first.z);
        break;
    }
    case TRANSFORM:
    {
        Poly::Polyhedron p = solid_in(in);
        float m[16];
        for (float& v : m) v = in.f();
        Poly::Transform(p, DirectX::XMMATRIX(m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9], m[10], m[11], m[12],
                                             m[13], m[14], m[15]));
        out.i(op); out.i(0); solid_out(out, p);
        break;
    }
    case KDOP:
    {
        std::vector<Vector3> pts = points_in(in);
        std::vector<Vector3> normals = points_in(in);
        const int ach = in.i();
        const double maxAxisScale = in.d();
        const float gapInv = in.f();
        Kdop::KdopContainer kdop(normals);
        if (ach)
            kdop.Calc(pts, maxAxisScale, gapInv);
        else
        {
            Poly::Polyhedron cloud(pts.size());
            for (size_t v = 0; v < pts.size(); ++v) cloud[v].Position = pts[v];
            kdop.Calc(cloud);
        }
        out.i(op); out.i(0);
        out.u((uint32_t)kdop.ElementVec.size());
        for (const Kdop::KdopElement& e : kdop.ElementVec)
        {
            out.f(e.MinPlane.x); out.f(e.MinPlane.y); out.f(e.MinPlane.z); out.f(e.MinPlane.w);
            out.f(e.MaxPlane.x); out.f(e.MaxPlane.y); out.f(e.MaxPlane.z); out.f(e.MaxPlane.w);
        }
        break;
    }
    case REFIT:
    {
        // The refitting step of the reference's event loop: hull normals of the Mesh under the point limit, the k-DOP of
        // the Mesh over them, and the Convex clipped by it.
        Poly::Polyhedron convex = solid_in(in);
        Poly::Polyhedron mesh = solid_in(in);
        const int limit = in.i();
        std::vector<Vector3> pts(mesh.size());
        for (size_t v = 0; v < mesh.size(); ++v) pts[v] = mesh[v].Position;
        Kdop::KdopContainer kdop(hull_normals(pts, std::min((int)mesh.size(), limit)));
        kdop.Calc(mesh);
        Poly::Polyhedron res = kdop.ClipWithPolyhedron(convex);
        out.i(op); out.i(0); solid_out(out, res);
        break;
    }
    case HULL:
    {
        std::vector<Vector3> pts = points_in(in);
        const int limit = in.i();
        std::vector<Vector3> n = hull_normals(pts, limit);
        out.i(op); out.i(0);
        out.u((uint32_t)n.size());
        for (const Vector3& v : n) { out.f(v.x); out.f(v.y); out.f(v.z); }
        break;
    }
    default:
        std::fprintf(stderr, "unknown op %d\n", op);
        std::exit(3);
    }
}

} // namespace

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: ref_driver <batch file> <result file>\n"); return 3; }
    In in;
    {
        FILE* fp = std::fopen(argv[1], "rb");
        if (!fp) { std::perror(argv[1]); return 3; }
        uint32_t v;
        while (std::fread(&v, 4, 1, fp) == 1) in.w.push_back(v);
        std::fclose(fp);
    }
    Out out;
    out.fp = std::fopen(argv[2], "wb");
    if (!out.fp) { std::perror(argv[2]); return 3; }
    const uint32_t n = in.u();
    for (uint32_t c = 0; c < n; ++c)
    {
        run_case(in, out);
        std::fflush(out.fp);
    }
    std::fclose(out.fp);
    return 0;
}
