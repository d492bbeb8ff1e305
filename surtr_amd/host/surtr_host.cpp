// surtr_host.cpp -- see surtr_host.hpp.  Flatten -> C ABI -> rebuild; no geometry here.
#include "surtr_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <random>

namespace surtr {

namespace {
struct Flat
{
    std::vector<uint32_t> vert_off{0}, nbr_off{0};
    std::vector<float> pos;
    std::vector<int32_t> nbr;
    void add(const Poly::Polyhedron& p)
    {
        for (const auto& v : p)
        {
            pos.push_back(v.Position.x); pos.push_back(v.Position.y); pos.push_back(v.Position.z);
            for (int a : v.NeighborVertexVec) nbr.push_back(a);
            nbr_off.push_back((uint32_t)nbr.size());
        }
        vert_off.push_back((uint32_t)(pos.size() / 3));
    }
};
Poly::Polyhedron rebuild(const float* pos, const uint32_t* off, const int32_t* nbr, uint32_t v0, uint32_t v1)
{
    Poly::Polyhedron p(v1 - v0);
    for (uint32_t v = v0; v < v1; ++v)
    {
        p[v - v0].Position = Vector3(pos[3 * v], pos[3 * v + 1], pos[3 * v + 2]);
        p[v - v0].NeighborVertexVec.assign(nbr + off[v], nbr + off[v + 1]);
    }
    return p;
}
} // namespace

namespace {
int g_default_device = 0;
std::vector<float> flat_points(const std::vector<Vector3>& v)
{
    std::vector<float> pts; pts.reserve(3 * v.size());
    for (const auto& p : v) { pts.push_back(p.x); pts.push_back(p.y); pts.push_back(p.z); }
    return pts;
}
} // namespace

void SetDefaultDevice(int device) { g_default_device = device; }
FractureEngine& DefaultEngine()
{
    static FractureEngine engine(g_default_device);
    return engine;
}

// ---- VMACH: the cell container ------------------------------------------------------------------------------------
Plane VMACH::ConstructFacePlane(const PolygonFace& f)
{
    if (f.VertexVec.size() < 3) throw Error(SURTR_E_INVALID, "ConstructFacePlane: face with fewer than 3 vertices");
    const float a[3] = {f.VertexVec[0].x, f.VertexVec[0].y, f.VertexVec[0].z}, b[3] = {f.VertexVec[1].x, f.VertexVec[1].y, f.VertexVec[1].z},
                c[3] = {f.VertexVec[2].x, f.VertexVec[2].y, f.VertexVec[2].z};
    float pl[4];
    surtr_plane_from_points(a, b, c, pl);
    return Plane(pl[0], pl[1], pl[2], pl[3]);
}
void VMACH::PolygonFace::ConstructFacePlane()
{
    if (GuaranteeConvex && VertexVec.size() >= 3) { FacePlane = VMACH::ConstructFacePlane(*this); FacePlaneConstructed = true; }
}
void VMACH::PolygonFace::AddVertex(const Vector3& v)
{
    // NearlyEqual: (v1 - v2).Length() < 1e-12 on floats, i.e. practically exact equality (Src/VMACH.cpp:1205, Inc/pch.h:18)
    for (const auto& o : VertexVec)
    {
        const float dx = o.x - v.x, dy = o.y - v.y, dz = o.z - v.z;
        if ((double)(dx * dx + dy * dy + dz * dz) < 1e-24) return;
    }
    VertexVec.push_back(v);
    if (GuaranteeConvex && VertexVec.size() == 3) ConstructFacePlane();
}
Vector3 VMACH::PolygonFace::GetNormal() const
{
    if (!FacePlaneConstructed) throw Error(SURTR_E_STATE, "PolygonFace::GetNormal: the face plane was never built (Src/VMACH.cpp:88-97)");
    return Vector3(FacePlane.x, FacePlane.y, FacePlane.z);      // already unit length
}
void VMACH::Polygon3D::Translate(const Vector3& t)
{
    for (auto& f : FaceVec) { for (auto& v : f.VertexVec) { v.x += t.x; v.y += t.y; v.z += t.z; } f.ConstructFacePlane(); }
}
void VMACH::Polygon3D::Scale(const Vector3& s)
{
    for (auto& f : FaceVec) { for (auto& v : f.VertexVec) { v.x *= s.x; v.y *= s.y; v.z *= s.z; } f.ConstructFacePlane(); }
}

// ---- Poly: free functions with the reference's signatures, on the default engine -------------------------------------
void Poly::InitPolyhedron(Polyhedron& polyhedron, const std::vector<Vector3>& positionVec, const std::vector<std::vector<int>>& neighborVec)
{
    polyhedron.resize(positionVec.size());
    for (size_t i = 0; i < positionVec.size(); ++i) { polyhedron[i].Position = positionVec[i]; polyhedron[i].NeighborVertexVec = neighborVec[i]; }
}

void Poly::Moments(double& zerothMoment, Vector3& firstMoment, const Polyhedron& polyhedron)
{
    Flat in; in.add(polyhedron);
    float cen[3] = {0, 0, 0};
    const int rc = surtr_moments((uint32_t)polyhedron.size(), in.pos.data(), in.nbr_off.data(), in.nbr.data(), &zerothMoment, cen);
    if (rc) throw Error(rc, std::string("Moments: ") + surtr_strerror(rc));
    firstMoment = Vector3(cen[0], cen[1], cen[2]);
}

Poly::Extract* Poly::ExtractFaces(const Polyhedron& polyhedron) { return new Extract(DefaultEngine().ExtractFaces(polyhedron)); }

void Poly::ClipPolyhedron(Polyhedron& polyhedron, const std::vector<Plane>& planes)
{
    if (polyhedron.empty()) return;
    polyhedron = DefaultEngine().ClipPolyhedron(polyhedron, planes);
}
Poly::Polyhedron Poly::ClipPolyhedron(const Polyhedron& polyhedron, const VMACH::Polygon3D& polygon3D)
{
    return DefaultEngine().ClipPolyhedron(polyhedron, polygon3D);
}
void Poly::Transform(Polyhedron& polyhedron, const Matrix& matrix) { polyhedron = DefaultEngine().TransformSolid(polyhedron, matrix); }

void Poly::RenderPolyhedron(std::vector<VertexNormalColor>& vertexData, std::vector<uint32_t>& indexData, const Polyhedron& poly,
                            const Extract* extract, bool isConvex, Vector3 color)
{
    (void)extract;      // == ExtractFaces(poly): the kernels derive the face loops themselves
    const FragmentRender r = DefaultEngine().RenderPolyhedron(poly, isConvex, color);
    const uint32_t vertexOffset = (uint32_t)vertexData.size();
    vertexData.insert(vertexData.end(), r.vertexData.begin(), r.vertexData.end());
    for (uint32_t i : r.indexData) indexData.push_back(vertexOffset + i);
}

void Poly::RenderPolyhedronNormal(std::vector<VertexNormalColor>& vertexData, std::vector<uint32_t>& indexData, const Polyhedron& poly, bool isConvex,
                                  Vector3 color)
{
    const FragmentRender r = DefaultEngine().RenderPolyhedronNormal(poly, isConvex, color);
    const uint32_t vertexOffset = (uint32_t)vertexData.size();
    vertexData.insert(vertexData.end(), r.vertexData.begin(), r.vertexData.end());
    for (uint32_t i : r.indexData) indexData.push_back(vertexOffset + i);
}
void Poly::RenderPolyhedronNormal(std::vector<VertexNormalColor>& vertexData, std::vector<uint32_t>& indexData, const Polyhedron& poly,
                                  const Extract* extract, bool isConvex, Vector3 color)
{
    (void)extract;      // == ExtractFaces(poly): the kernels derive the face loops themselves
    RenderPolyhedronNormal(vertexData, indexData, poly, isConvex, color);
}

// ---- Kdop ------------------------------------------------------------------------------------------------------------
Kdop::KdopContainer::KdopContainer(const std::vector<Vector3>& normalVec)
{
    for (const auto& n : normalVec) ElementVec.emplace_back(n);
}
namespace {
void fill_kdop(Kdop::KdopContainer& K, const std::vector<float>& pts, bool ach, double maxAxisScale, float planeGapInv)
{
    const uint32_t k = (uint32_t)K.ElementVec.size(), n = (uint32_t)(pts.size() / 3);
    if (k == 0 || n == 0) return;
    std::vector<float> nrm, pl(8 * (size_t)k);
    for (const auto& e : K.ElementVec) { nrm.push_back(e.Normal.x); nrm.push_back(e.Normal.y); nrm.push_back(e.Normal.z); }
    const int rc = ach ? surtr_kdop_ach_planes(n, pts.data(), k, nrm.data(), maxAxisScale, planeGapInv, pl.data())
                       : surtr_kdop_planes(n, pts.data(), k, nrm.data(), pl.data());
    if (rc) throw Error(rc, std::string("KdopContainer::Calc: ") + surtr_strerror(rc));
    for (uint32_t j = 0; j < k; ++j)
    {
        K.ElementVec[j].MinPlane = Plane(pl[8 * j], pl[8 * j + 1], pl[8 * j + 2], pl[8 * j + 3]);
        K.ElementVec[j].MaxPlane = Plane(pl[8 * j + 4], pl[8 * j + 5], pl[8 * j + 6], pl[8 * j + 7]);
    }
}
} // namespace
void Kdop::KdopContainer::Calc(const std::vector<Vector3>& vertices, const double& maxAxisScale, const float& planeGapInv)
{
    fill_kdop(*this, flat_points(vertices), true, maxAxisScale, planeGapInv);
}
void Kdop::KdopContainer::Calc(const Poly::Polyhedron& mesh)
{
    std::vector<float> pts;
    for (const auto& v : mesh) { pts.push_back(v.Position.x); pts.push_back(v.Position.y); pts.push_back(v.Position.z); }
    fill_kdop(*this, pts, false, 0.0, 1.f);
}
Poly::Polyhedron Kdop::KdopContainer::ClipWithPolyhedron(const Poly::Polyhedron& polyhedron)
{
    std::vector<Plane> planes;
    for (const auto& e : ElementVec) { planes.push_back(e.MinPlane); planes.push_back(e.MaxPlane); }
    Poly::Polyhedron res = polyhedron;
    Poly::ClipPolyhedron(res, planes);
    return res;
}

std::vector<Vector3> GenerateICHNormal(const std::vector<Vector3>& vertices, int limitCnt)
{
    const std::vector<float> pts = flat_points(vertices);
    uint32_t k = 0;
    int rc = surtr_hull_normals((uint32_t)vertices.size(), pts.data(), (uint32_t)limitCnt, 0, nullptr, &k);
    if (rc) throw Error(rc, std::string("GenerateICHNormal: ") + surtr_strerror(rc));
    std::vector<float> nrm(3 * (size_t)k + 3);
    rc = surtr_hull_normals((uint32_t)vertices.size(), pts.data(), (uint32_t)limitCnt, k, nrm.data(), &k);
    if (rc) throw Error(rc, std::string("GenerateICHNormal: ") + surtr_strerror(rc));
    std::vector<Vector3> out(k);
    for (uint32_t i = 0; i < k; ++i) out[i] = Vector3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
    return out;
}

Poly::Polyhedron Poly::GetBB()
{
    static const float P[8][3] = {{-.5f, -.5f, -.5f}, {.5f, -.5f, -.5f}, {.5f, .5f, -.5f}, {-.5f, .5f, -.5f},
                                  {-.5f, -.5f, .5f},  {.5f, -.5f, .5f},  {.5f, .5f, .5f},  {-.5f, .5f, .5f}};
    static const int NB[8][3] = {{1, 4, 3}, {5, 0, 2}, {3, 6, 1}, {7, 2, 0}, {5, 7, 0}, {1, 6, 4}, {5, 2, 7}, {4, 6, 3}};
    Polyhedron p(8);
    for (int i = 0; i < 8; ++i) { p[i].Position = Vector3(P[i][0], P[i][1], P[i][2]); p[i].NeighborVertexVec.assign(NB[i], NB[i] + 3); }
    return p;
}

void Poly::Translate(Polyhedron& polyhedron, const Vector3& v)
{
    for (auto& i : polyhedron) { i.Position.x += v.x; i.Position.y += v.y; i.Position.z += v.z; }
}

void Poly::Scale(Polyhedron& polyhedron, const Vector3& v)
{
    for (auto& i : polyhedron) { i.Position.x *= v.x; i.Position.y *= v.y; i.Position.z *= v.z; }
}

std::vector<std::vector<int>> Poly::ExtractNeighborFromMesh(std::vector<Vector3>& vertices, std::vector<int>& indices)
{
    // on the device (surtr_neighbors_from_mesh_dev: directed-edge hash + one fan walk per vertex; same rings, same refusals)
    const uint32_t nv = (uint32_t)vertices.size(), nt = (uint32_t)(indices.size() / 3);
    std::vector<uint32_t> off(nv + 1);
    std::vector<int32_t> nbr(6 * (size_t)nt + 1);
    std::vector<int32_t> tris(indices.begin(), indices.end());
    const int rc = surtr_neighbors_from_mesh_dev(DefaultEngine().Raw(), nv, nt, tris.data(), off.data(), nbr.data(), nullptr);
    if (rc) throw Error(rc, std::string("ExtractNeighborFromMesh: ") + surtr_strerror(rc));
    std::vector<std::vector<int>> out(nv);
    for (uint32_t v = 0; v < nv; ++v) out[v].assign(nbr.begin() + off[v], nbr.begin() + off[v + 1]);
    return out;
}

FractureEngine::FractureEngine(int device) { check(surtr_create(device, &ctx_), "surtr_create"); }
FractureEngine::~FractureEngine() { surtr_destroy(ctx_); }

void LoadModelData(const std::string& fileName, const Vector3& scale, const Vector3& translate, std::vector<Vector3>& vertices,
                   std::vector<int>& indices)
{
    const float sc[3] = {scale.x, scale.y, scale.z}, tr[3] = {translate.x, translate.y, translate.z};
    uint32_t nv = 0, nt = 0;
    int rc = surtr_read_obj(fileName.c_str(), sc, tr, 0, 0, nullptr, nullptr, &nv, &nt);
    if (rc) throw Error(rc, "LoadModelData: cannot read " + fileName);
    std::vector<float> pos(3 * (size_t)nv + 3); std::vector<int32_t> tri(3 * (size_t)nt + 3);
    rc = surtr_read_obj(fileName.c_str(), sc, tr, nv, nt, pos.data(), tri.data(), &nv, &nt);
    if (rc) throw Error(rc, "LoadModelData: cannot read " + fileName);
    vertices.resize(nv); indices.assign(tri.begin(), tri.begin() + 3 * (size_t)nt);
    for (uint32_t v = 0; v < nv; ++v) vertices[v] = Vector3(pos[3 * v], pos[3 * v + 1], pos[3 * v + 2]);
}

Poly::Polyhedron FractureEngine::BuildACH(const std::vector<Vector3>& vertices, uint32_t ichIncludePointLimit, float achPlaneGapInverse)
{
    if (vertices.empty()) throw Error(SURTR_E_INVALID, "BuildACH: no vertices");
    std::vector<float> pts; pts.reserve(3 * vertices.size());
    Vector3 lo = vertices[0], hi = vertices[0];
    for (const auto& p : vertices)
    {
        pts.push_back(p.x); pts.push_back(p.y); pts.push_back(p.z);
        lo.x = std::min(lo.x, p.x); hi.x = std::max(hi.x, p.x); lo.y = std::min(lo.y, p.y); hi.y = std::max(hi.y, p.y);
        lo.z = std::min(lo.z, p.z); hi.z = std::max(hi.z, p.z);
    }
    // steps 1-2: ICH face normals
    std::vector<float> nrm(3 * (size_t)(2 * ichIncludePointLimit + 8));
    uint32_t k = 0;
    check(surtr_hull_normals((uint32_t)vertices.size(), pts.data(), ichIncludePointLimit, (uint32_t)(nrm.size() / 3), nrm.data(), &k), "surtr_hull_normals");
    // steps 3-4: bounding box, k-DOP min/max planes
    const double maxAxis = std::max(std::max((double)hi.x - lo.x, (double)hi.y - lo.y), (double)hi.z - lo.z);
    std::vector<float> pl(8 * (size_t)k);
    check(surtr_kdop_ach_planes((uint32_t)vertices.size(), pts.data(), k, nrm.data(), maxAxis, achPlaneGapInverse, pl.data()), "surtr_kdop_ach_planes");
    // steps 5-6: 2x box, clipped by every plane
    Poly::Polyhedron box = Poly::GetBB();
    Poly::Scale(box, Vector3(hi.x - lo.x, hi.y - lo.y, hi.z - lo.z)); Poly::Scale(box, Vector3(2, 2, 2));
    Poly::Translate(box, Vector3((float)(((double)hi.x + lo.x) / 2.0), (float)(((double)hi.y + lo.y) / 2.0), (float)(((double)hi.z + lo.z) / 2.0)));
    std::vector<Plane> planes(2 * (size_t)k);
    for (size_t i = 0; i < planes.size(); ++i) { planes[i].x = pl[4 * i]; planes[i].y = pl[4 * i + 1]; planes[i].z = pl[4 * i + 2]; planes[i].w = pl[4 * i + 3]; }
    return ClipPolyhedron(box, planes);
}

std::vector<Fragment> FractureEngine::PrepareFracture(std::vector<Vector3>& vertices, std::vector<int>& indices, const std::vector<Vector3>& cellPointVec)
{
    Piece piece;
    piece.Convex = BuildACH(vertices);
    Poly::InitPolyhedron(piece.Mesh, vertices, Poly::ExtractNeighborFromMesh(vertices, indices));      // step 7
    Vector3 lo = vertices[0], hi = vertices[0];
    for (const auto& p : vertices)
    {
        lo.x = std::min(lo.x, p.x); hi.x = std::max(hi.x, p.x); lo.y = std::min(lo.y, p.y); hi.y = std::max(hi.y, p.y);
        lo.z = std::min(lo.z, p.z); hi.z = std::max(hi.z, p.z);
    }
    SetPattern(GenerateVoronoi(cellPointVec));                                                          // step 8
    PlacePattern(Vector3(hi.x - lo.x, hi.y - lo.y, hi.z - lo.z),
                 Vector3((float)(((double)hi.x + lo.x) / 2.0), (float)(((double)hi.y + lo.y) / 2.0), (float)(((double)hi.z + lo.z) / 2.0)));
    Compound comp; comp.PieceVec.push_back(piece);
    SetCompound(comp);
    return ApplyFracture();                                                                             // step 10 (+ Refitting, SetExtract)
}

void FractureEngine::check(int rc, const char* what)
{
    if (rc) throw Error(rc, std::string(what) + ": " + surtr_strerror(rc) + " " + (ctx_ ? surtr_last_error(ctx_) : ""));
}

void FractureEngine::SetPattern(const std::vector<VMACH::Polygon3D>& voroPolyVec)
{
    std::vector<uint32_t> face_off{0};
    std::vector<float> v012;
    for (const auto& cell : voroPolyVec)
    {
        for (const auto& f : cell.FaceVec)
        {
            if (f.VertexVec.size() < 3) throw Error(SURTR_E_INVALID, "face with fewer than 3 vertices");
            for (int k = 0; k < 3; ++k) { v012.push_back(f.VertexVec[k].x); v012.push_back(f.VertexVec[k].y); v012.push_back(f.VertexVec[k].z); }
        }
        face_off.push_back((uint32_t)(v012.size() / 9));
    }
    n_cells_ = (uint32_t)voroPolyVec.size();
    installed_id_ = -1;
    check(surtr_upload_pattern(ctx_, n_cells_, face_off.data(), v012.data()), "surtr_upload_pattern");
}

std::vector<VMACH::Polygon3D> FractureEngine::GenerateVoronoiHost(const std::vector<Vector3>& cellPointVec)
{
    const uint32_t n = (uint32_t)cellPointVec.size();
    std::vector<double> seeds;
    for (const auto& s : cellPointVec) { seeds.push_back(s.x); seeds.push_back(s.y); seeds.push_back(s.z); }
    uint32_t nf = 0, nfv = 0;
    int rc = surtr_voronoi_cells(n, seeds.data(), &nf, &nfv, nullptr, nullptr, nullptr, nullptr);
    if (rc) throw Error(rc, "surtr_voronoi_cells");
    std::vector<uint32_t> cfo(n + 1), fvo(nf + 1);
    std::vector<int32_t> gen(nf);
    std::vector<double> verts(3 * (size_t)nfv);
    rc = surtr_voronoi_cells(n, seeds.data(), &nf, &nfv, cfo.data(), gen.data(), fvo.data(), verts.data());
    if (rc) throw Error(rc, "surtr_voronoi_cells");
    std::vector<VMACH::Polygon3D> out(n);
    for (uint32_t c = 0; c < n; ++c)
        for (uint32_t f = cfo[c]; f < cfo[c + 1]; ++f)
        {
            VMACH::PolygonFace face(true);
            for (uint32_t v = fvo[f]; v < fvo[f + 1]; ++v)
                face.VertexVec.emplace_back((float)verts[3 * v], (float)verts[3 * v + 1], (float)verts[3 * v + 2]);
            face.ConstructFacePlane();
            out[c].FaceVec.push_back(face);
        }
    return out;
}

std::vector<VMACH::Polygon3D> FractureEngine::GenerateVoronoi(const std::vector<Vector3>& cellPointVec)
{
    const uint32_t n = (uint32_t)cellPointVec.size();
    std::vector<double> seeds;
    for (const auto& s : cellPointVec) { seeds.push_back(s.x); seeds.push_back(s.y); seeds.push_back(s.z); }
    const uint32_t group_off[2] = {0u, n};
    uint32_t nf = 0, nfv = 0;
    check(surtr_build_cells(ctx_, 1, group_off, seeds.data(), &nf, &nfv), "surtr_build_cells");
    n_cells_ = n;                                       // the cells are this engine's pattern now
    installed_id_ = -1;
    std::vector<uint32_t> cfo(n + 1), fvo(nf + 1);
    std::vector<double> verts(3 * (size_t)nfv + 3);
    check(surtr_download_cells(ctx_, cfo.data(), nullptr, fvo.data(), verts.data(), nullptr), "surtr_download_cells");
    std::vector<VMACH::Polygon3D> out(n);
    for (uint32_t c = 0; c < n; ++c)
        for (uint32_t f = cfo[c]; f < cfo[c + 1]; ++f)
        {
            VMACH::PolygonFace face(true);
            for (uint32_t v = fvo[f]; v < fvo[f + 1]; ++v)
                face.VertexVec.emplace_back((float)verts[3 * v], (float)verts[3 * v + 1], (float)verts[3 * v + 2]);
            face.ConstructFacePlane();
            out[c].FaceVec.push_back(face);
        }
    return out;
}

std::vector<VMACH::Polygon3D> FractureEngine::GenerateVoronoi(int cellCnt, int seed)
{
    // Src/Surtr.cpp:1984-2001 (libstdc++'s distributions, like the oracle's and surtr_amd/scenes.py)
    std::mt19937 gen((unsigned)seed);
    std::uniform_real_distribution<double> uniformDist(-0.5, 0.5);
    std::vector<Vector3> cellPointVec;
    for (int i = 0; i < cellCnt; ++i)
    {
        const double x = uniformDist(gen), y = uniformDist(gen), z = uniformDist(gen);
        cellPointVec.emplace_back((float)x, (float)y, (float)z);
    }
    return GenerateVoronoi(cellPointVec);
}

std::vector<VMACH::Polygon3D> FractureEngine::GenerateFracturePattern(int cellCount, double mean, int seed)
{
    // Src/Surtr.cpp:2072-2096
    std::mt19937 gen((unsigned)seed);
    std::uniform_real_distribution<double> directionUniformDist(-1.0, 1.0);
    std::exponential_distribution<double> lengthExpDist(1.0 / mean);
    std::vector<Vector3> cellPointVec;
    for (int i = 0; i < cellCount; ++i)
    {
        const double len = std::max(std::min(lengthExpDist(gen), 0.5), 1e-12);
        const double x = directionUniformDist(gen), y = directionUniformDist(gen), z = directionUniformDist(gen);
        Vector3 v((float)x, (float)y, (float)z);
        const float t = v.x * v.x + v.y * v.y;
        const float l = std::sqrt(t + v.z * v.z);                                 // Vector3::Normalize: divide by sqrt(dot)
        v.x = v.x / l; v.y = v.y / l; v.z = v.z / l;
        const float fl = (float)len;                                              // v *= len (XMVectorScale by a float)
        v.x *= fl; v.y *= fl; v.z *= fl;
        cellPointVec.push_back(v);
    }
    return GenerateVoronoi(cellPointVec);
}

void FractureEngine::PlacePattern(const Vector3& scale, const Vector3& translate)
{
    const float s[3] = {scale.x, scale.y, scale.z}, t[3] = {translate.x, translate.y, translate.z};
    check(surtr_place_cells(ctx_, s, t), "surtr_place_cells");
}

int FractureEngine::StorePattern()
{
    uint32_t id = 0;
    check(surtr_pattern_store(ctx_, &id), "surtr_pattern_store");
    installed_id_ = (int)id;
    return (int)id;
}

void FractureEngine::SelectPattern(int id)
{
    if (id < 0) throw Error(SURTR_E_INVALID, "SelectPattern: no such pattern");
    uint32_t nc = 0;
    check(surtr_pattern_info(ctx_, (uint32_t)id, &nc, nullptr), "surtr_pattern_info");
    check(surtr_pattern_select(ctx_, (uint32_t)id), "surtr_pattern_select");
    n_cells_ = nc; installed_id_ = id;
}

int FractureEngine::PatternCount()
{
    uint32_t n = 0;
    check(surtr_pattern_count(ctx_, &n), "surtr_pattern_count");
    return (int)n;
}

void FractureEngine::ClearPatterns()
{
    check(surtr_pattern_clear(ctx_), "surtr_pattern_clear");
    installed_id_ = pair_partial_ = pair_general_ = -1;
}

int FractureEngine::installed_pattern_id() { return installed_id_ >= 0 ? installed_id_ : StorePattern(); }

// (before the installed pattern is stored for the impacts that name none: that store must not make a wrong id a right one)
void FractureEngine::check_impact_patterns(const std::vector<Impact>& impacts)
{
    const int n = PatternCount();
    for (const Impact& im : impacts)
        if (im.pattern >= n) throw Error(SURTR_E_INVALID, "Impact::pattern " + std::to_string(im.pattern) + ": " + std::to_string(n) + " patterns are stored");
}

std::pair<int, int> FractureEngine::PrepareFracturePatterns(const FractureArgs& args)
{
    GenerateFracturePattern(args.PartialFracturePatternCellCnt, args.PartialFracturePatternDist, args.Seed);
    const int partialId = StorePattern();
    GenerateFracturePattern(args.GeneralFracturePatternCellCnt, args.GeneralFracturePatternDist, args.Seed);
    return {partialId, StorePattern()};
}

void FractureEngine::UsePatternPair(int partialId, int generalId)
{
    if ((partialId < 0) != (generalId < 0) || partialId >= PatternCount() || generalId >= PatternCount()) throw Error(SURTR_E_INVALID, "UsePatternPair: no such pattern");
    pair_partial_ = partialId; pair_general_ = generalId;
}

void FractureEngine::SetCompound(const Compound& compound)
{
    Flat m, c;
    for (const auto& p : compound.PieceVec) { m.add(p.Mesh); c.add(p.Convex); }
    n_pieces_ = (uint32_t)compound.PieceVec.size();
    check(surtr_upload_pieces(ctx_, n_pieces_, m.vert_off.data(), m.pos.data(), m.nbr_off.data(), m.nbr.data(),
                              c.vert_off.data(), c.pos.data(), c.nbr_off.data(), c.nbr.data()), "surtr_upload_pieces");
}

std::vector<Fragment> FractureEngine::ApplyFracture(const std::set<int>& outside, bool refit, bool render, uint32_t cellBegin, uint32_t cellEnd)
{
    std::vector<uint8_t> mask(n_pieces_, 0);
    for (int o : outside) if (o >= 0 && (uint32_t)o < n_pieces_) mask[o] = 1;
    if (cellEnd == 0xFFFFFFFFu) cellEnd = n_cells_;
    const uint32_t flags = (refit ? SURTR_EVT_REFIT : 0u) | (render ? SURTR_EVT_RENDER : 0u);
    check(surtr_fracture_event(ctx_, cellBegin, cellEnd, outside.empty() ? nullptr : mask.data(), flags, &counts_), "surtr_fracture_event");
    std::vector<Fragment> out = download_fragments(render);
    report_flagged(out, cellBegin, cellEnd, "ApplyFracture");
    return out;
}

// What the event flagged (surtr_counts::n_failed): the pairs without a fragment from surtr_pair_status (pair = (cell - cellBegin)
// * pieces + piece, the order of the reference's double loop, Src/Surtr.cpp:1457-1504), the fragments from their status word.
void FractureEngine::report_flagged(const std::vector<Fragment>& frags, uint32_t cellBegin, uint32_t cellEnd, const char* what)
{
    flagged_ = FlaggedUnits();
    flagged_.n_failed = counts_.n_failed;
    if (counts_.n_failed == 0) return;
    for (size_t f = 0; f < frags.size(); ++f) if (frags[f].status != 0) flagged_.fragments.push_back((uint32_t)f);
    const uint32_t n_pairs = (cellEnd - cellBegin) * n_pieces_;
    std::vector<uint32_t> st(n_pairs);
    if (n_pairs != 0 && surtr_pair_status(ctx_, n_pairs, st.data()) == SURTR_OK)
        for (uint32_t p = 0; p < n_pairs; ++p)
            if (st[p] != 0) flagged_.pairs.emplace_back((int)(cellBegin + p / n_pieces_), (int)(p % n_pieces_));
    if (!allow_flagged_)
        throw Error(SURTR_E_TOPOLOGY, std::string(what) + ": " + std::to_string(flagged_.pairs.size()) + " (cell, piece) pair(s) without a valid clip and " +
                    std::to_string(flagged_.fragments.size()) + " fragment(s) flagged (input outside the reference's domain; AllowFlagged(true) returns the rest)");
}

std::vector<Fragment> FractureEngine::download_fragments(bool render)
{
    const surtr_counts& c = counts_;
    std::vector<int32_t> ids(3 * (size_t)c.n_frag), mnbr(c.mesh_nbrs), cnbr(c.conv_nbrs);
    std::vector<uint32_t> mvo(c.n_frag + 1), mno(c.mesh_verts + 1), cvo(c.n_frag + 1), cno(c.conv_verts + 1), ioff(c.n_frag + 1), idx(c.n_idx);
    std::vector<float> mpos(3 * (size_t)c.mesh_verts), cpos(3 * (size_t)c.conv_verts), vnc(9 * (size_t)c.mesh_verts);
    std::vector<uint32_t> fstat(c.n_frag);
    surtr_fragments fr{ids.data(), mvo.data(), mpos.data(), mno.data(), mnbr.data(), cvo.data(), cpos.data(), cno.data(), cnbr.data(),
                       vnc.data(), ioff.data(), idx.data(), fstat.data()};
    check(surtr_event_download(ctx_, &fr), "surtr_event_download");
    std::vector<Fragment> out(c.n_frag);
    for (uint32_t f = 0; f < c.n_frag; ++f)
    {
        Fragment& F = out[f];
        F.cell = ids[3 * f]; F.piece = ids[3 * f + 1]; F.island = ids[3 * f + 2]; F.status = (int)fstat[f];
        F.piece_data.Mesh = rebuild(mpos.data(), mno.data(), mnbr.data(), mvo[f], mvo[f + 1]);
        // rings are fragment-local already; offsets are global over the vertex array
        F.piece_data.Convex = rebuild(cpos.data(), cno.data(), cnbr.data(), cvo[f], cvo[f + 1]);
        if (render && c.n_idx != 0)
        {
            F.render.vertexData.resize(mvo[f + 1] - mvo[f]);
            std::memcpy(F.render.vertexData.data(), vnc.data() + 9 * (size_t)mvo[f], sizeof(VertexNormalColor) * F.render.vertexData.size());
            F.render.indexData.assign(idx.begin() + ioff[f], idx.begin() + ioff[f + 1]);
        }
    }
    return out;
}

Poly::Polyhedron FractureEngine::ClipPolyhedron(const Poly::Polyhedron& polyhedron, const std::vector<Plane>& planes)
{
    if (polyhedron.size() < 4) return Poly::Polyhedron();      // fewer than four vertices: the reference's answer is the empty solid (Src/Poly.cpp:497-499)
    Flat in; in.add(polyhedron);
    std::vector<float> pl;
    for (const auto& p : planes) { pl.push_back(p.x); pl.push_back(p.y); pl.push_back(p.z); pl.push_back(p.w); }
    uint32_t nv = 0, nh = 0;
    const uint32_t V = (uint32_t)polyhedron.size();
    check(surtr_clip_polyhedron(ctx_, V, in.pos.data(), in.nbr_off.data(), in.nbr.data(), (uint32_t)planes.size(), pl.data(), &nv, &nh,
                                nullptr, nullptr, nullptr), "surtr_clip_polyhedron");
    std::vector<float> pos(3 * (size_t)nv + 3); std::vector<uint32_t> off(nv + 1); std::vector<int32_t> nbr(nh + 1);
    check(surtr_clip_polyhedron(ctx_, V, in.pos.data(), in.nbr_off.data(), in.nbr.data(), (uint32_t)planes.size(), pl.data(), &nv, &nh,
                                pos.data(), off.data(), nbr.data()), "surtr_clip_polyhedron");
    return rebuild(pos.data(), off.data(), nbr.data(), 0, nv);
}

Poly::Polyhedron FractureEngine::ClipPolyhedron(const Poly::Polyhedron& polyhedron, const VMACH::Polygon3D& polygon3D)
{
    // The reference keeps PolygonFace::FacePlane current through ConstructFacePlane on AddVertex / Scale / Translate
    // (Src/VMACH.cpp:302-310); this layer's PolygonFace is a plain struct, so the plane is rebuilt here from the first three
    // vertices with the arithmetic of k_place_cells (Plane(p0,p1,p2), normalised: SimpleMath.inl:2773-2780).
    std::vector<Plane> planes;
    for (const auto& f : polygon3D.FaceVec)
    {
        if (f.VertexVec.size() < 3) throw Error(SURTR_E_INVALID, "ClipPolyhedron: face with fewer than 3 vertices");
        planes.push_back(VMACH::ConstructFacePlane(f));
    }
    return ClipPolyhedron(polyhedron, planes);
}

void FractureEngine::TransformCompound(const std::vector<Matrix>& worldMatrices)
{
    if (worldMatrices.size() != n_pieces_) throw Error(SURTR_E_INVALID, "TransformCompound: one matrix per piece");
    std::vector<float> w; w.reserve(16 * worldMatrices.size());
    for (const auto& m : worldMatrices) w.insert(w.end(), m.m, m.m + 16);
    check(surtr_transform_pieces(ctx_, n_pieces_, w.data()), "surtr_transform_pieces");
}

uint32_t FractureEngine::CompoundFromLastEvent(const std::vector<uint8_t>& keep)
{
    uint32_t n = 0;
    check(surtr_pieces_from_event(ctx_, keep.empty() ? nullptr : keep.data(), &n), "surtr_pieces_from_event");
    n_pieces_ = n;
    return n;
}

void FractureEngine::Refitting(std::vector<Piece>& pieceVec)
{
    if (pieceVec.empty()) return;
    Flat m, c;
    for (const auto& p : pieceVec) { m.add(p.Mesh); c.add(p.Convex); }
    const uint32_t n = (uint32_t)pieceVec.size();
    check(surtr_load_fragments(ctx_, n, m.vert_off.data(), m.pos.data(), m.nbr_off.data(), m.nbr.data(),
                               c.vert_off.data(), c.pos.data(), c.nbr_off.data(), c.nbr.data(), nullptr), "surtr_load_fragments");
    check(surtr_event_refit(ctx_), "surtr_event_refit");
    check(surtr_event_counts(ctx_, &counts_), "surtr_event_counts");
    std::vector<uint32_t> cvo(n + 1), cno(counts_.conv_verts + 1);
    std::vector<float> cpos(3 * (size_t)counts_.conv_verts + 3);
    std::vector<int32_t> cnbr(counts_.conv_nbrs + 1);
    surtr_fragments fr{};
    fr.conv_vert_off = cvo.data(); fr.conv_pos = cpos.data(); fr.conv_nbr_off = cno.data(); fr.conv_nbr = cnbr.data();
    check(surtr_event_download(ctx_, &fr), "surtr_event_download");
    for (uint32_t k = 0; k < n; ++k) pieceVec[k].Convex = rebuild(cpos.data(), cno.data(), cnbr.data(), cvo[k], cvo[k + 1]);
}

std::vector<surtr_mass> FractureEngine::MassProperties(int set, float density)
{
    uint32_t n = 0;
    check(surtr_event_mass(ctx_, set, density, &n, nullptr), "surtr_event_mass");
    std::vector<surtr_mass> out(n);
    if (n) check(surtr_event_mass(ctx_, set, density, &n, out.data()), "surtr_event_mass");
    return out;
}

namespace {
template <class F>
HullSet hulls_of(F call, const char* what)
{
    HullSet h;
    uint32_t n = 0, np = 0, ni = 0;
    int rc = call(&n, nullptr, &np, nullptr, &ni, nullptr);
    if (rc) throw Error(rc, what);
    h.Records.resize(n); h.Polygons.resize(np); h.Indices.resize(ni);
    // (the fill form wants three arrays: empty vectors lend it a place to stand)
    surtr_hull r0; surtr_hull_polygon p0; uint16_t i0;
    rc = call(&n, n ? h.Records.data() : &r0, &np, np ? h.Polygons.data() : &p0, &ni, ni ? h.Indices.data() : &i0);
    if (rc) throw Error(rc, what);
    return h;
}
}

HullSet FractureEngine::Hulls()
{
    return hulls_of([&](uint32_t* n, surtr_hull* r, uint32_t* np, surtr_hull_polygon* p, uint32_t* ni, uint16_t* i) { return surtr_event_hulls(ctx_, n, r, np, p, ni, i); },
                    "surtr_event_hulls");
}

std::vector<FragmentRender> FractureEngine::ShadedRender(const Vector3& color, std::vector<surtr_shaded>* records)
{
    const float col[3] = {color.x, color.y, color.z};
    uint32_t n = 0, nv = 0, nf = 0;
    check(surtr_event_shaded(ctx_, col, &n, nullptr, &nv, nullptr, nullptr, &nf), "surtr_event_shaded");
    // (the fill form wants both arrays: empty vectors lend it a place to stand)
    std::vector<surtr_shaded> rec(std::max(n, 1u)); std::vector<VertexNormalColor> vnc(std::max(nv, 1u));
    check(surtr_event_shaded(ctx_, col, &n, rec.data(), &nv, (float*)vnc.data(), nullptr, &nf), "surtr_event_shaded");
    rec.resize(n);
    std::vector<FragmentRender> out(n);
    for (uint32_t f = 0; f < n; ++f)
    {
        out[f].vertexData.assign(vnc.begin() + rec[f].first_vertex, vnc.begin() + rec[f].first_vertex + rec[f].n_vertices);
        out[f].indexData.resize(rec[f].n_vertices);
        for (uint32_t i = 0; i < rec[f].n_vertices; ++i) out[f].indexData[i] = i;
    }
    if (records) *records = std::move(rec);
    return out;
}

FragmentRender FractureEngine::RenderPolyhedronNormal(const Poly::Polyhedron& poly, bool isConvex, const Vector3& color)
{
    Flat in; in.add(poly);
    uint32_t ni = 0;
    check(surtr_triangulate(ctx_, (uint32_t)poly.size(), in.pos.data(), in.nbr_off.data(), in.nbr.data(), isConvex ? 1 : 0, nullptr, nullptr, &ni, nullptr),
          "surtr_triangulate");
    return std::move(ShadedRender(color).front());
}

HullSet FractureEngine::PieceHulls()
{
    return hulls_of([&](uint32_t* n, surtr_hull* r, uint32_t* np, surtr_hull_polygon* p, uint32_t* ni, uint16_t* i) { return surtr_pieces_hulls(ctx_, n, r, np, p, ni, i); },
                    "surtr_pieces_hulls");
}

namespace {
template <class F>
CookedSet cooked_of(const HullSet* hulls, F call, const char* what)
{
    CookedSet c;
    const surtr_hull* hr = hulls && !hulls->Records.empty() ? hulls->Records.data() : nullptr;
    const uint32_t nh = hulls ? (uint32_t)hulls->Records.size() : 0u;
    uint32_t n = 0, nv = 0, np = 0, ni = 0;
    int rc = call(hr, nh, &n, nullptr, &nv, nullptr, nullptr, &np, nullptr, &ni, nullptr);
    if (rc) throw Error(rc, what);
    c.Records.resize(n); c.Points.resize(3 * (size_t)nv); c.Source.resize(nv); c.Polygons.resize(np); c.Indices.resize(ni);
    surtr_cooked r0; float f0[3]; uint32_t s0; surtr_hull_polygon p0; uint16_t i0;
    rc = call(hr, nh, &n, n ? c.Records.data() : &r0, &nv, nv ? c.Points.data() : f0, nv ? c.Source.data() : &s0, &np, np ? c.Polygons.data() : &p0, &ni,
              ni ? c.Indices.data() : &i0);
    if (rc) throw Error(rc, what);
    return c;
}
}

CookedSet FractureEngine::CookHulls(bool unusableOnly, float relTol, float weldDistance, float planeTolerance)
{
    HullSet h;
    if (unusableOnly) h = Hulls();
    return cooked_of(unusableOnly ? &h : nullptr, [&](const surtr_hull* hr, uint32_t nh, uint32_t* n, surtr_cooked* r, uint32_t* nv, float* pts, uint32_t* src,
                                                      uint32_t* np, surtr_hull_polygon* p, uint32_t* ni, uint16_t* i) {
        return surtr_event_cook(ctx_, hr, nh, relTol, weldDistance, planeTolerance, n, r, nv, pts, src, np, p, ni, i); }, "surtr_event_cook");
}

CookedSet FractureEngine::CookPieceHulls(bool unusableOnly, float relTol, float weldDistance, float planeTolerance)
{
    HullSet h;
    if (unusableOnly) h = PieceHulls();
    return cooked_of(unusableOnly ? &h : nullptr, [&](const surtr_hull* hr, uint32_t nh, uint32_t* n, surtr_cooked* r, uint32_t* nv, float* pts, uint32_t* src,
                                                      uint32_t* np, surtr_hull_polygon* p, uint32_t* ni, uint16_t* i) {
        return surtr_pieces_cook(ctx_, hr, nh, relTol, weldDistance, planeTolerance, n, r, nv, pts, src, np, p, ni, i); }, "surtr_pieces_cook");
}

std::vector<Poly::Extract> FractureEngine::SetExtract()
{
    const HullSet h = Hulls();
    std::vector<Poly::Extract> out(h.Records.size());
    for (size_t k = 0; k < h.Records.size(); ++k)
    {
        const surtr_hull& r = h.Records[k];
        for (uint32_t f = 0; f < r.n_faces; ++f)
        {
            const surtr_hull_polygon& p = h.Polygons[r.face_off + f];
            const uint16_t* q = h.Indices.data() + r.idx_off + p.index_base;
            out[k].emplace_back(q, q + p.n_verts);
        }
    }
    return out;
}

std::vector<surtr_mass> FractureEngine::PieceMassProperties(int set, float density)
{
    uint32_t n = 0;
    check(surtr_pieces_mass(ctx_, set, density, &n, nullptr), "surtr_pieces_mass");
    std::vector<surtr_mass> out(n);
    if (n) check(surtr_pieces_mass(ctx_, set, density, &n, out.data()), "surtr_pieces_mass");
    return out;
}

surtr_ray_hit FractureEngine::Raycast(const Vector3& origin, const Vector3& dir, float maxDist)
{
    const float ray[7] = {origin.x, origin.y, origin.z, dir.x, dir.y, dir.z, maxDist};
    surtr_ray_hit hit;
    check(surtr_pieces_raycast(ctx_, 1, ray, &hit), "surtr_pieces_raycast");
    return hit;
}

std::vector<uint8_t> FractureEngine::OverlapSphere(const Vector3& centre, float radius, float minMass)
{
    const float sphere[4] = {centre.x, centre.y, centre.z, radius};
    uint32_t n = 0;
    check(surtr_pieces_overlap(ctx_, 1, sphere, nullptr, 0.f, &n, nullptr), "surtr_pieces_overlap");
    std::vector<uint8_t> mask(n);
    std::vector<surtr_mass> mass;
    if (minMass >= 0.f) mass = PieceMassProperties(1);
    check(surtr_pieces_overlap(ctx_, 1, sphere, mass.empty() ? nullptr : mass.data(), minMass, &n, mask.data()), "surtr_pieces_overlap");
    return mask;
}

std::vector<int> FractureEngine::PickImpact(const Vector3& origin, const Vector3& dir, FractureArgs& args, const std::vector<int>& pieceCompound)
{
    const surtr_ray_hit hit = Raycast(origin, dir);
    if (hit.piece < 0) return {};
    if ((size_t)hit.piece >= pieceCompound.size()) throw Error(SURTR_E_INVALID, "PickImpact: pieceCompound is shorter than the resident pieces");
    args.ImpactPosition = Vector3(hit.pos[0] + dir.x * args.TargetAdder, hit.pos[1] + dir.y * args.TargetAdder, hit.pos[2] + dir.z * args.TargetAdder);
    if (!args.RadialMode) return {pieceCompound[hit.piece]};
    const std::vector<uint8_t> mask = OverlapSphere(args.ImpactPosition, args.ImpactRadius / 2.f, 1e-4f);
    if (mask.size() > pieceCompound.size()) throw Error(SURTR_E_INVALID, "PickImpact: pieceCompound is shorter than the resident pieces");
    std::set<int> out;
    for (size_t p = 0; p < mask.size(); ++p) if (mask[p] == 1) out.insert(pieceCompound[p]);
    return std::vector<int>(out.begin(), out.end());
}

void FractureEngine::SetScene(const std::vector<Compound>& compoundVec)
{
    Compound all;
    std::vector<uint32_t> off(1, 0u);
    for (const auto& c : compoundVec)
    {
        if (c.PieceVec.empty()) throw Error(SURTR_E_INVALID, "SetScene: a compound without pieces");
        all.PieceVec.insert(all.PieceVec.end(), c.PieceVec.begin(), c.PieceVec.end());
        off.push_back((uint32_t)all.PieceVec.size());
    }
    if (compoundVec.empty()) throw Error(SURTR_E_INVALID, "SetScene: no compound");
    SetCompound(all);
    check(surtr_scene_set_compounds(ctx_, (uint32_t)compoundVec.size(), off.data()), "surtr_scene_set_compounds");
}

std::vector<uint32_t> FractureEngine::SceneCompounds()
{
    uint32_t n = 0;
    check(surtr_scene_get_compounds(ctx_, 0, &n, nullptr), "surtr_scene_get_compounds");
    std::vector<uint32_t> off(n + 1);
    check(surtr_scene_get_compounds(ctx_, n + 1, &n, off.data()), "surtr_scene_get_compounds");
    return off;
}

std::vector<int> FractureEngine::PickImpact(const Vector3& origin, const Vector3& dir, FractureArgs& args)
{
    const std::vector<uint32_t> off = SceneCompounds();
    std::vector<int> pieceCompound(off.back());
    for (size_t c = 0; c + 1 < off.size(); ++c) for (uint32_t p = off[c]; p < off[c + 1]; ++p) pieceCompound[p] = (int)c;
    return PickImpact(origin, dir, args, pieceCompound);
}

// DoFracture's cloud (:1911-1915): every point scaled by the radius, then moved to the impact; flat, three floats per point.
std::vector<float> FractureEngine::placed_cloud(const std::vector<Vector3>& spherePointCloud, float radius, const Vector3& position)
{
    std::vector<Vector3> cloud = spherePointCloud;
    for (auto& v : cloud)
    {
        v.x *= radius; v.y *= radius; v.z *= radius;
        v.x += position.x; v.y += position.y; v.z += position.z;
    }
    return flat_points(cloud);
}

// The end of every ExecuteFractureRoutine: the regrouping (sizes, then the compounds; a call without bodies leaves nb at one), the
// refit, the flagged check, the commit.  -> the compounds made.
std::vector<int> FractureEngine::regroup_refit_commit(const char* what, const std::function<int(uint32_t*, uint32_t*, uint32_t*, int32_t*, uint32_t*, uint32_t*)>& regroup)
{
    uint32_t np = 0, nc = 0, nb = 1;
    check(regroup(&np, &nc, nullptr, nullptr, &nb, nullptr), what);
    std::vector<uint32_t> off((size_t)np + nb + 1), body(nb + 1);
    std::vector<int32_t> piece(np + 1);
    check(regroup(&np, &nc, off.data(), piece.data(), &nb, body.data()), what);
    check(surtr_event_refit(ctx_), "surtr_event_refit");
    check(surtr_event_counts(ctx_, &counts_), "surtr_event_counts");
    flagged_ = FlaggedUnits();
    flagged_.n_failed = counts_.n_failed;
    if (counts_.n_failed && !allow_flagged_)
        throw Error(SURTR_E_TOPOLOGY, "ExecuteFractureRoutine: the event flagged " + std::to_string(counts_.n_failed) + " unit(s); nothing was committed");
    uint32_t n = 0, first = 0, n_new = 0;
    check(surtr_scene_commit(ctx_, nc, off.data(), piece.data(), &n, &first, &n_new, nullptr), "surtr_scene_commit");
    n_pieces_ = n;
    std::vector<int> made(n_new);
    for (uint32_t k = 0; k < n_new; ++k) made[k] = (int)(first + k);
    return made;
}

// The loop of one-compound routines of OnMouseDown / OnMouseDownBodies, in DESCENDING number: a commit moves only the compounds above its
// target, and those have been dealt with.
std::vector<int> FractureEngine::fracture_descending(const std::vector<int>& hit, float maxAxisScale, const FractureArgs& args,
                                                     const std::vector<Vector3>& spherePointCloud)
{
    std::vector<int> made;
    for (auto it = hit.rbegin(); it != hit.rend(); ++it)
    {
        for (int& c : made) --c;      // (the compounds made so far sit above every target still to come: each moves down by one)
        const std::vector<int> more = ExecuteFractureRoutine(*it, {}, maxAxisScale, args, spherePointCloud);
        made.insert(made.end(), more.begin(), more.end());
    }
    return made;
}

// Count-then-fill of a byte mask: call(cap, &n, bytes).
std::vector<uint8_t> FractureEngine::two_call_mask(const char* what, const std::function<int(uint32_t, uint32_t*, uint8_t*)>& call)
{
    uint32_t n = 0;
    check(call(0, &n, nullptr), what);
    std::vector<uint8_t> mask(n + 1);
    check(call(n, &n, mask.data()), what);
    mask.resize(n);
    return mask;
}

std::vector<int> FractureEngine::ExecuteFractureRoutine(int compound, const std::vector<Matrix>& world, float maxAxisScale, const FractureArgs& args,
                                                        const std::vector<Vector3>& spherePointCloud)
{
    const std::vector<uint32_t> table = SceneCompounds();
    if (compound < 0 || (size_t)compound + 1 >= table.size()) throw Error(SURTR_E_INVALID, "ExecuteFractureRoutine: no such compound");
    const uint32_t p0 = table[(size_t)compound], m = table[(size_t)compound + 1] - p0;
    // the pre-transform (:1846-1851)
    if (!world.empty())
    {
        if (world.size() != m) throw Error(SURTR_E_INVALID, "ExecuteFractureRoutine: one matrix per piece of the compound");
        std::vector<float> w; w.reserve(16 * world.size());
        for (const auto& x : world) w.insert(w.end(), x.m, x.m + 16);
        check(surtr_scene_transform_compound(ctx_, (uint32_t)compound, m, w.data()), "surtr_scene_transform_compound");
    }
    else ApplyPose(compound);      // the pose the scene holds for this body (the identity: nothing)
    // DoFracture's placement (:1890-1915)
    const float s2 = maxAxisScale * 2.f;
    SetRefittingPointLimit(args.RefittingPointLimit);
    PlacePattern(Vector3(s2, s2, s2), args.ImpactPosition);
    const std::vector<float> fc = placed_cloud(spherePointCloud, args.ImpactRadius, args.ImpactPosition);
    const float org[3] = {args.ImpactPosition.x, args.ImpactPosition.y, args.ImpactPosition.z};
    // the pieces of the compound out of the sphere are kept whole
    std::vector<uint8_t> mask(m, 0);
    bool any = false;
    for (uint32_t k = 0; args.PartialFracture && k < m; ++k)
    {
        uint32_t nv = 0, nh = 0;
        check(surtr_download_piece(ctx_, p0 + k, 1, &nv, &nh, nullptr, nullptr, nullptr), "surtr_download_piece");
        std::vector<float> pos(3 * (size_t)nv + 3); std::vector<uint32_t> no(nv + 1); std::vector<int32_t> nbr(nh + 1);
        check(surtr_download_piece(ctx_, p0 + k, 1, &nv, &nh, pos.data(), no.data(), nbr.data()), "surtr_download_piece");
        int out = 0;
        const int rc = surtr_convex_out_of_sphere(nv, pos.data(), no.data(), nbr.data(), (uint32_t)(fc.size() / 3), fc.data(), org, args.ImpactRadius, &out);
        if (rc) throw Error(rc, std::string("surtr_convex_out_of_sphere: ") + surtr_strerror(rc));
        mask[k] = out ? 1 : 0; any = any || out;
    }
    check(surtr_scene_fracture_event(ctx_, (uint32_t)compound, 0, n_cells_, any ? mask.data() : nullptr, 0u, &counts_), "surtr_scene_fracture_event");
    const int partial = args.PartialFracture ? 1 : 0;
    return regroup_refit_commit("surtr_event_regroup", [&](uint32_t* np, uint32_t* nc, uint32_t* off, int32_t* piece, uint32_t*, uint32_t*) {
        return surtr_event_regroup(ctx_, partial, (uint32_t)(fc.size() / 3), fc.data(), org, args.ImpactRadius, np, nc, off, piece);
    });
}

static std::vector<uint32_t> compound_numbers(const std::vector<int>& compounds, const char* who)
{
    std::vector<uint32_t> out;
    for (int c : compounds)
    {
        if (c < 0) throw Error(SURTR_E_INVALID, std::string(who) + ": no such compound");
        out.push_back((uint32_t)c);
    }
    return out;
}

std::vector<uint8_t> FractureEngine::outside_mask(const std::vector<uint32_t>& t, const std::vector<float>& fc, const float org[3], float radius)
{
    return two_call_mask("surtr_scene_outside", [&](uint32_t cap, uint32_t* n, uint8_t* bytes) {
        return surtr_scene_outside(ctx_, (uint32_t)t.size(), t.data(), (uint32_t)(fc.size() / 3), fc.data(), org, radius, cap, n, bytes);
    });
}

std::vector<uint8_t> FractureEngine::OutsideMask(const std::vector<int>& compounds, const FractureArgs& args, const std::vector<Vector3>& cloud)
{
    const float org[3] = {args.ImpactPosition.x, args.ImpactPosition.y, args.ImpactPosition.z};
    return outside_mask(compound_numbers(compounds, "OutsideMask"), flat_points(cloud), org, args.ImpactRadius);
}

std::vector<int> FractureEngine::ExecuteFractureRoutine(const std::vector<int>& compounds, float maxAxisScale, const FractureArgs& args,
                                                        const std::vector<Vector3>& spherePointCloud)
{
    std::vector<int> sorted(compounds);
    std::sort(sorted.begin(), sorted.end(), [](int a, int b) { return a > b; });
    if (sorted.empty()) throw Error(SURTR_E_INVALID, "ExecuteFractureRoutine: no compound");
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) throw Error(SURTR_E_INVALID, "ExecuteFractureRoutine: a compound is named twice");
    const std::vector<uint32_t> t = compound_numbers(sorted, "ExecuteFractureRoutine");
    ApplyPoses(sorted);
    // DoFracture's placement (:1890-1915)
    const float s2 = maxAxisScale * 2.f;
    SetRefittingPointLimit(args.RefittingPointLimit);
    PlacePattern(Vector3(s2, s2, s2), args.ImpactPosition);
    const std::vector<float> fc = placed_cloud(spherePointCloud, args.ImpactRadius, args.ImpactPosition);
    const float org[3] = {args.ImpactPosition.x, args.ImpactPosition.y, args.ImpactPosition.z};
    std::vector<uint8_t> mask;
    if (args.PartialFracture) mask = outside_mask(t, fc, org, args.ImpactRadius);
    const bool any = std::find_if(mask.begin(), mask.end(), [](uint8_t o) { return o != 0; }) != mask.end();
    check(surtr_scene_fracture_bodies(ctx_, (uint32_t)t.size(), t.data(), 0, n_cells_, any ? mask.data() : nullptr, 0u, &counts_), "surtr_scene_fracture_bodies");
    const int partial = args.PartialFracture ? 1 : 0;
    return regroup_refit_commit("surtr_event_regroup_bodies", [&](uint32_t* np, uint32_t* nc, uint32_t* off, int32_t* piece, uint32_t* nb, uint32_t* body) {
        return surtr_event_regroup_bodies(ctx_, partial, (uint32_t)(fc.size() / 3), fc.data(), org, args.ImpactRadius, np, nc, off, piece, nb, body);
    });
}

std::vector<int> FractureEngine::OnMouseDown(const Vector3& origin, const Vector3& dir, FractureArgs& args, float maxAxisScale,
                                             const std::vector<Vector3>& spherePointCloud, std::vector<int>* hitCompounds, bool oneEvent)
{
    std::vector<int> hit = PickImpact(origin, dir, args);
    if (hitCompounds) *hitCompounds = hit;
    if (oneEvent) return hit.empty() ? std::vector<int>() : ExecuteFractureRoutine(hit, maxAxisScale, args, spherePointCloud);
    return fracture_descending(hit, maxAxisScale, args, spherePointCloud);
}

void FractureEngine::SetPoses(const std::vector<Matrix>& world)
{
    std::vector<float> w; w.reserve(16 * world.size());
    for (const auto& x : world) w.insert(w.end(), x.m, x.m + 16);
    check(surtr_scene_set_poses(ctx_, (uint32_t)world.size(), w.data()), "surtr_scene_set_poses");
}

std::vector<Matrix> FractureEngine::Poses()
{
    uint32_t n = 0;
    check(surtr_scene_get_poses(ctx_, 0, &n, nullptr), "surtr_scene_get_poses");
    std::vector<float> w(16 * (size_t)n + 16);
    check(surtr_scene_get_poses(ctx_, n, &n, w.data()), "surtr_scene_get_poses");
    std::vector<Matrix> out(n);
    for (uint32_t c = 0; c < n; ++c) std::copy(w.begin() + 16 * (size_t)c, w.begin() + 16 * (size_t)(c + 1), out[c].m);
    return out;
}

void FractureEngine::ApplyPose(int compound)
{
    if (compound < 0) throw Error(SURTR_E_INVALID, "ApplyPose: no such compound");
    check(surtr_scene_apply_pose(ctx_, (uint32_t)compound), "surtr_scene_apply_pose");
}

void FractureEngine::ApplyPoses(const std::vector<int>& compounds)
{
    const std::vector<uint32_t> t = compound_numbers(compounds, "ApplyPoses");
    check(surtr_scene_apply_poses(ctx_, (uint32_t)t.size(), t.data()), "surtr_scene_apply_poses");
}

surtr_scene_ray_hit FractureEngine::RaycastScene(const Vector3& origin, const Vector3& dir, float maxDist)
{
    const float ray[7] = {origin.x, origin.y, origin.z, dir.x, dir.y, dir.z, maxDist};
    surtr_scene_ray_hit hit;
    check(surtr_scene_raycast(ctx_, 1, ray, &hit), "surtr_scene_raycast");
    return hit;
}

std::vector<surtr_mass> FractureEngine::BodyMassProperties(int set, float density)
{
    uint32_t n = 0;
    check(surtr_scene_mass(ctx_, set, density, &n, nullptr), "surtr_scene_mass");
    std::vector<surtr_mass> out(n);
    if (n) check(surtr_scene_mass(ctx_, set, density, &n, out.data()), "surtr_scene_mass");
    return out;
}

std::vector<surtr_bounds> FractureEngine::BodyBounds(int set)
{
    uint32_t n = 0;
    check(surtr_scene_bounds(ctx_, set, &n, nullptr), "surtr_scene_bounds");
    std::vector<surtr_bounds> out(n);
    if (n) check(surtr_scene_bounds(ctx_, set, &n, out.data()), "surtr_scene_bounds");
    return out;
}

std::vector<surtr_contact> FractureEngine::Contacts(float margin, surtr_contact_header* totals)
{
    if (totals) check(surtr_scene_contacts_totals(ctx_, margin, totals), "surtr_scene_contacts_totals");
    uint32_t n = 0;
    check(surtr_scene_contacts(ctx_, margin, &n, nullptr), "surtr_scene_contacts");
    std::vector<surtr_contact> out(n);
    if (n) check(surtr_scene_contacts(ctx_, margin, &n, out.data()), "surtr_scene_contacts");
    return out;
}

std::vector<Impact> ImpactsFromContacts(const std::vector<surtr_contact>& contacts, float radius)
{
    std::vector<Impact> out;
    std::vector<size_t> best;      // per impact: the record it stands for
    for (size_t i = 0; i < contacts.size(); ++i)
    {
        const surtr_contact& r = contacts[i];
        size_t k = 0;
        while (k < out.size() && !(contacts[best[k]].body_a == r.body_a && contacts[best[k]].body_b == r.body_b)) ++k;
        if (k == out.size()) { out.push_back(Impact{}); best.push_back(i); }
        else if (!(r.distance < contacts[best[k]].distance)) continue;
        else best[k] = i;
        Impact& im = out[k];
        im.position = Vector3((r.point_a[0] + r.point_b[0]) * 0.5f, (r.point_a[1] + r.point_b[1]) * 0.5f, (r.point_a[2] + r.point_b[2]) * 0.5f);
        im.radius = radius;
        im.compounds = {(int)r.body_a, (int)r.body_b};
    }
    return out;
}

void FractureEngine::RemoveBodies(const std::vector<int>& compounds)
{
    std::vector<uint32_t> t;
    for (int c : compounds)
    {
        if (c < 0) throw Error(SURTR_E_INVALID, "RemoveBodies: no such compound");
        t.push_back((uint32_t)c);
    }
    uint32_t n = n_pieces_;
    check(surtr_scene_remove(ctx_, (uint32_t)t.size(), t.data(), &n, nullptr), "surtr_scene_remove");
    n_pieces_ = n;
}

int FractureEngine::AddBodies(const std::vector<Compound>& compoundVec, const std::vector<Matrix>& poses)
{
    if (compoundVec.empty()) throw Error(SURTR_E_INVALID, "AddBodies: no compound");
    if (!poses.empty() && poses.size() != compoundVec.size()) throw Error(SURTR_E_INVALID, "AddBodies: one pose per compound");
    Flat m, c;
    std::vector<uint32_t> off(1, 0u);
    for (const auto& comp : compoundVec)
    {
        if (comp.PieceVec.empty()) throw Error(SURTR_E_INVALID, "AddBodies: a compound without pieces");
        for (const auto& p : comp.PieceVec) { m.add(p.Mesh); c.add(p.Convex); }
        off.push_back(off.back() + (uint32_t)comp.PieceVec.size());
    }
    std::vector<float> w;
    for (const auto& x : poses) w.insert(w.end(), x.m, x.m + 16);
    uint32_t first = 0;
    check(surtr_scene_append(ctx_, (uint32_t)compoundVec.size(), off.data(), m.vert_off.data(), m.pos.data(), m.nbr_off.data(), m.nbr.data(),
                             c.vert_off.data(), c.pos.data(), c.nbr_off.data(), c.nbr.data(), w.empty() ? nullptr : w.data(), &first), "surtr_scene_append");
    n_pieces_ += off.back();
    return (int)first;
}

std::vector<uint8_t> FractureEngine::CullBodies(float minMass, const std::pair<Vector3, Vector3>* keepBox, bool apply)
{
    float box[6] = {};
    if (keepBox) { box[0] = keepBox->first.x; box[1] = keepBox->first.y; box[2] = keepBox->first.z; box[3] = keepBox->second.x; box[4] = keepBox->second.y; box[5] = keepBox->second.z; }
    // (minMass < 0: no body is light -- a mass record with status 0 has a positive volume)
    uint32_t n = 0, removed = 0;
    check(surtr_scene_cull(ctx_, 1, 10.f, minMass, keepBox ? box : nullptr, 0, &n, nullptr, &removed), "surtr_scene_cull");
    std::vector<uint8_t> reason(n);
    check(surtr_scene_cull(ctx_, 1, 10.f, minMass, keepBox ? box : nullptr, apply ? 1 : 0, &n, reason.data(), &removed), "surtr_scene_cull");
    if (removed) n_pieces_ = SceneCompounds().back();
    return reason;
}

std::vector<uint8_t> FractureEngine::OverlapBodies(const Vector3& centre, float radius, float minMass)
{
    const float sphere[4] = {centre.x, centre.y, centre.z, radius};
    uint32_t n = 0;
    check(surtr_scene_overlap(ctx_, 1, sphere, nullptr, 0.f, &n, nullptr), "surtr_scene_overlap");
    std::vector<uint8_t> mask(n);
    std::vector<surtr_mass> mass;
    if (minMass >= 0.f) mass = BodyMassProperties(1);
    check(surtr_scene_overlap(ctx_, 1, sphere, mass.empty() ? nullptr : mass.data(), minMass, &n, mask.data()), "surtr_scene_overlap");
    return mask;
}

std::vector<int> FractureEngine::PickBodies(const Vector3& origin, const Vector3& dir, FractureArgs& args, surtr_scene_ray_hit* hitOut,
                                            std::vector<uint8_t>* bodyMask)
{
    const surtr_scene_ray_hit hit = RaycastScene(origin, dir);
    if (hitOut) *hitOut = hit;
    if (bodyMask) bodyMask->clear();
    if (hit.piece < 0) return {};
    args.ImpactPosition = Vector3(hit.pos[0] + dir.x * args.TargetAdder, hit.pos[1] + dir.y * args.TargetAdder, hit.pos[2] + dir.z * args.TargetAdder);
    if (!args.RadialMode && !bodyMask) return {hit.compound};
    const std::vector<uint8_t> mask = OverlapBodies(args.ImpactPosition, args.ImpactRadius / 2.f, 1e-4f);
    if (bodyMask) *bodyMask = mask;
    if (!args.RadialMode) return {hit.compound};
    std::vector<int> out;
    for (size_t c = 0; c < mask.size(); ++c) if (mask[c] == 1) out.push_back((int)c);
    return out;
}

std::vector<std::vector<InitCompoundResult>> FractureEngine::InitCompounds(const std::vector<int>& compounds, bool renderConvex, bool withHulls, bool cookUnusable,
                                                                           const FractureArgs& cookArgs)
{
    if (cookUnusable && !withHulls) throw Error(SURTR_E_INVALID, "InitCompounds: cookUnusable needs withHulls");
    std::vector<std::vector<InitCompoundResult>> out;
    if (compounds.empty()) return out;
    std::vector<uint32_t> list;
    for (int c : compounds) { if (c < 0) throw Error(SURTR_E_INVALID, "InitCompounds: no such compound"); list.push_back((uint32_t)c); }
    const std::vector<uint32_t> table = SceneCompounds();
    check(surtr_scene_fragments(ctx_, (uint32_t)list.size(), list.data(), renderConvex ? 1 : 0, SURTR_EVT_RENDER, &counts_), "surtr_scene_fragments");
    const surtr_counts& c = counts_;
    // only what the two consumers take: the Convex points, the render buffers, the status words
    std::vector<uint32_t> mvo(c.n_frag + 1), cvo(c.n_frag + 1), ioff(c.n_frag + 1), idx(c.n_idx), fstat(c.n_frag);
    std::vector<float> cpos(3 * (size_t)c.conv_verts), vnc(9 * (size_t)c.mesh_verts);
    surtr_fragments fr{};
    fr.mesh_vert_off = mvo.data(); fr.conv_vert_off = cvo.data(); fr.conv_pos = cpos.data(); fr.vnc = vnc.data(); fr.idx_off = ioff.data(); fr.idx = idx.data();
    fr.frag_status = fstat.data();
    check(surtr_event_download(ctx_, &fr), "surtr_event_download");
    flagged_ = FlaggedUnits();
    flagged_.n_failed = c.n_failed;
    for (uint32_t f = 0; f < c.n_frag; ++f) if (fstat[f] != 0) flagged_.fragments.push_back(f);
    if (c.n_failed != 0 && !allow_flagged_)
        throw Error(SURTR_E_TOPOLOGY, "InitCompounds: " + std::to_string(flagged_.fragments.size()) +
                    " piece(s) flagged (their faces cannot be extracted; AllowFlagged(true) returns the rest)");
    HullSet hulls;
    CookedSet cooked;
    if (cookUnusable)
    {
        // both answers from one call: arrays at the bounds that are always enough, cut to what was written
        uint32_t n = c.n_frag, hp = std::max(c.conv_nbrs, 1u), hi = hp, nv = std::max(c.conv_verts, 1u), np = 2 * nv, ni = 6 * nv;
        hulls.Records.resize(std::max(n, 1u)); hulls.Polygons.resize(hp); hulls.Indices.resize(hi);
        cooked.Records.resize(std::max(n, 1u)); cooked.Points.resize(3 * (size_t)nv); cooked.Source.resize(nv); cooked.Polygons.resize(np); cooked.Indices.resize(ni);
        check(surtr_event_hulls_cook(ctx_, cookArgs.HullRelTolerance, cookArgs.CookWeldDistance, cookArgs.CookPlaneTolerance, &n, hulls.Records.data(), &hp,
                                     hulls.Polygons.data(), &hi, hulls.Indices.data(), cooked.Records.data(), &nv, cooked.Points.data(), cooked.Source.data(), &np,
                                     cooked.Polygons.data(), &ni, cooked.Indices.data()), "surtr_event_hulls_cook");
        hulls.Records.resize(n); hulls.Polygons.resize(hp); hulls.Indices.resize(hi);
        cooked.Records.resize(n); cooked.Points.resize(3 * (size_t)nv); cooked.Source.resize(nv); cooked.Polygons.resize(np); cooked.Indices.resize(ni);
    }
    else if (withHulls) hulls = Hulls();
    std::vector<FragmentRender> lit; std::vector<surtr_shaded> litRecords;
    if (render_normals_) lit = ShadedRender(Vector3(0.25f, 0.25f, 0.25f), &litRecords);
    uint32_t f = 0;
    for (uint32_t comp : list)
    {
        out.emplace_back();
        for (uint32_t p = table[comp]; p < table[comp + 1]; ++p, ++f)
        {
            InitCompoundResult r;
            for (uint32_t v = cvo[f]; v < cvo[f + 1]; ++v) r.ConvexPoints.emplace_back(cpos[3 * (size_t)v], cpos[3 * (size_t)v + 1], cpos[3 * (size_t)v + 2]);
            r.Mesh.vertexData.resize(mvo[f + 1] - mvo[f]);
            if (!r.Mesh.vertexData.empty()) std::memcpy(r.Mesh.vertexData.data(), vnc.data() + 9 * (size_t)mvo[f], sizeof(VertexNormalColor) * r.Mesh.vertexData.size());
            r.Mesh.indexData.assign(idx.begin() + ioff[f], idx.begin() + ioff[f + 1]);
            if (render_normals_) { r.MeshLit = std::move(lit[f]); r.Lit = litRecords[f]; }
            if (withHulls)
            {
                const surtr_hull& h = hulls.Records[f];
                r.Hull.Record = h;
                r.Hull.Polygons.assign(hulls.Polygons.begin() + h.face_off, hulls.Polygons.begin() + h.face_off + h.n_faces);
                r.Hull.Indices.assign(hulls.Indices.begin() + h.idx_off, hulls.Indices.begin() + h.idx_off + h.n_idx);
            }
            if (cookUnusable)
            {
                const surtr_cooked& k = cooked.Records[f];
                r.Cooked.Record = k;
                for (uint32_t v = k.pt_off; v < k.pt_off + k.nv; ++v) r.Cooked.Points.emplace_back(cooked.Points[3 * (size_t)v], cooked.Points[3 * (size_t)v + 1], cooked.Points[3 * (size_t)v + 2]);
                r.Cooked.Source.assign(cooked.Source.begin() + k.pt_off, cooked.Source.begin() + k.pt_off + k.nv);
                r.Cooked.Polygons.assign(cooked.Polygons.begin() + k.face_off, cooked.Polygons.begin() + k.face_off + k.n_faces);
                r.Cooked.Indices.assign(cooked.Indices.begin() + k.idx_off, cooked.Indices.begin() + k.idx_off + k.n_idx);
            }
            out.back().push_back(std::move(r));
        }
    }
    return out;
}

std::vector<InitCompoundResult> FractureEngine::InitCompound(int compound, bool renderConvex, bool withHulls)
{
    return std::move(InitCompounds(std::vector<int>{compound}, renderConvex, withHulls).front());
}

std::vector<int> FractureEngine::OnMouseDownBodies(const Vector3& origin, const Vector3& dir, FractureArgs& args, float maxAxisScale,
                                                   const std::vector<Vector3>& spherePointCloud, std::vector<int>* hitCompounds,
                                                   surtr_scene_ray_hit* hitOut, std::vector<uint8_t>* bodyMask, bool oneEvent)
{
    std::vector<int> hit = PickBodies(origin, dir, args, hitOut, bodyMask);
    if (hitCompounds) *hitCompounds = hit;
    if (oneEvent) return hit.empty() ? std::vector<int>() : ExecuteFractureRoutine(hit, maxAxisScale, args, spherePointCloud);
    return fracture_descending(hit, maxAxisScale, args, spherePointCloud);
}

std::vector<int> FractureEngine::ExecuteFractureRoutine(const std::vector<Impact>& impacts, float maxAxisScale, const FractureArgs& args,
                                                        const std::vector<Vector3>& spherePointCloud)
{
    if (impacts.empty()) throw Error(SURTR_E_INVALID, "ExecuteFractureRoutine: no impact");
    const uint32_t K = (uint32_t)impacts.size();
    std::vector<uint32_t> toff{0u}, t, soff{0u};
    std::vector<int> all;
    std::vector<float> scale3, shift3, rad, fc;
    const float s2 = maxAxisScale * 2.f;
    for (const Impact& im : impacts)
    {
        std::vector<int> sorted(im.compounds);
        std::sort(sorted.begin(), sorted.end(), [](int a, int b) { return a > b; });
        if (sorted.empty()) throw Error(SURTR_E_INVALID, "ExecuteFractureRoutine: an impact without a compound");
        const std::vector<uint32_t> tn = compound_numbers(sorted, "ExecuteFractureRoutine");
        t.insert(t.end(), tn.begin(), tn.end()); toff.push_back((uint32_t)t.size());
        all.insert(all.end(), sorted.begin(), sorted.end());
        // DoFracture's placement per impact (:1890-1915)
        scale3.insert(scale3.end(), {s2, s2, s2});
        shift3.insert(shift3.end(), {im.position.x, im.position.y, im.position.z});
        rad.push_back(im.radius);
        const std::vector<float> one = placed_cloud(spherePointCloud, im.radius, im.position);
        fc.insert(fc.end(), one.begin(), one.end()); soff.push_back((uint32_t)(fc.size() / 3));
    }
    {
        std::vector<int> s(all);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end()) throw Error(SURTR_E_INVALID, "ExecuteFractureRoutine: a compound is named twice");
    }
    ApplyPoses(all);
    SetRefittingPointLimit(args.RefittingPointLimit);
    if (fc.empty()) fc.assign(3, 0.f);
    if (std::find_if(impacts.begin(), impacts.end(), [](const Impact& im) { return im.pattern >= 0 || im.partial >= 0; }) != impacts.end())
    {
        // ---- the pattern library: a stored pattern and a flag per impact
        check_impact_patterns(impacts);
        std::vector<uint32_t> ids; std::vector<uint8_t> flags;
        for (const Impact& im : impacts)
        {
            ids.push_back((uint32_t)(im.pattern >= 0 ? im.pattern : installed_pattern_id()));
            flags.push_back(im.partial >= 0 ? (im.partial ? 1 : 0) : (args.PartialFracture ? 1 : 0));
        }
        check(surtr_place_cells_patterns(ctx_, K, ids.data(), scale3.data(), shift3.data()), "surtr_place_cells_patterns");
        uint32_t nb = 0;
        check(surtr_placed_cells(ctx_, 0, &nb, nullptr), "surtr_placed_cells");
        cell_base_.assign(nb, 0u);
        check(surtr_placed_cells(ctx_, nb, &nb, cell_base_.data()), "surtr_placed_cells");
        std::vector<uint8_t> lmask;
        if (std::find(flags.begin(), flags.end(), (uint8_t)1) != flags.end())
        {
            lmask = two_call_mask("surtr_scene_outside_impacts", [&](uint32_t cap, uint32_t* n, uint8_t* bytes) {
                return surtr_scene_outside_impacts(ctx_, K, toff.data(), t.data(), soff.data(), fc.data(), shift3.data(), rad.data(), cap, n, bytes);
            });
            // the bytes of the impacts that are not partial are cleared: their pieces are all broken
            const std::vector<uint32_t> table = SceneCompounds();
            size_t at = 0;
            for (uint32_t i = 0; i < K; ++i)
                for (uint32_t k = toff[i]; k < toff[i + 1]; ++k)
                {
                    const size_t m = table[(size_t)t[k] + 1] - table[t[k]];
                    if (!flags[i]) std::fill(lmask.begin() + at, lmask.begin() + at + m, (uint8_t)0);
                    at += m;
                }
        }
        const bool lany = std::find_if(lmask.begin(), lmask.end(), [](uint8_t o) { return o != 0; }) != lmask.end();
        check(surtr_scene_fracture_impacts(ctx_, K, toff.data(), t.data(), 0, SURTR_CELLS_ALL, lany ? lmask.data() : nullptr, 0u, &counts_), "surtr_scene_fracture_impacts");
        return regroup_refit_commit("surtr_event_regroup_impacts_partial", [&](uint32_t* np, uint32_t* nc, uint32_t* off, int32_t* piece, uint32_t* nbod, uint32_t* body) {
            return surtr_event_regroup_impacts_partial(ctx_, flags.data(), K, soff.data(), fc.data(), shift3.data(), rad.data(), np, nc, off, piece, nbod, body);
        });
    }
    check(surtr_place_cells_impacts(ctx_, K, scale3.data(), shift3.data()), "surtr_place_cells_impacts");
    std::vector<uint8_t> mask;
    if (args.PartialFracture)
        mask = two_call_mask("surtr_scene_outside_impacts", [&](uint32_t cap, uint32_t* n, uint8_t* bytes) {
            return surtr_scene_outside_impacts(ctx_, K, toff.data(), t.data(), soff.data(), fc.data(), shift3.data(), rad.data(), cap, n, bytes);
        });
    const bool any = std::find_if(mask.begin(), mask.end(), [](uint8_t o) { return o != 0; }) != mask.end();
    check(surtr_scene_fracture_impacts(ctx_, K, toff.data(), t.data(), 0, n_cells_, any ? mask.data() : nullptr, 0u, &counts_), "surtr_scene_fracture_impacts");
    const int partial = args.PartialFracture ? 1 : 0;
    return regroup_refit_commit("surtr_event_regroup_impacts", [&](uint32_t* np, uint32_t* nc, uint32_t* off, int32_t* piece, uint32_t* nb, uint32_t* body) {
        return surtr_event_regroup_impacts(ctx_, partial, K, soff.data(), fc.data(), shift3.data(), rad.data(), np, nc, off, piece, nb, body);
    });
}

std::vector<int> FractureEngine::OnImpacts(const std::vector<Impact>& spheres, const FractureArgs& args, float maxAxisScale,
                                           const std::vector<Vector3>& spherePointCloud, std::vector<Impact>* acted, bool oneEvent)
{
    if (acted) acted->clear();
    if (spheres.empty()) return {};
    // every sphere in one query, with PickBodies' radius and mass gate (:228)
    std::vector<float> q;
    for (const Impact& s : spheres) q.insert(q.end(), {s.position.x, s.position.y, s.position.z, s.radius / 2.f});
    uint32_t nc = 0;
    check(surtr_scene_overlap(ctx_, (uint32_t)spheres.size(), q.data(), nullptr, 0.f, &nc, nullptr), "surtr_scene_overlap");
    std::vector<uint8_t> mask((size_t)nc * spheres.size());
    const std::vector<surtr_mass> mass = BodyMassProperties(1);
    check(surtr_scene_overlap(ctx_, (uint32_t)spheres.size(), q.data(), mass.data(), 1e-4f, &nc, mask.data()), "surtr_scene_overlap");
    std::vector<uint8_t> taken(nc, 0);
    std::vector<Impact> impacts;
    for (size_t s = 0; s < spheres.size(); ++s)
    {
        Impact im = spheres[s];
        im.compounds.clear();
        for (uint32_t c = 0; c < nc; ++c)
            if (mask[s * nc + c] == 1 && !taken[c]) { taken[c] = 1; im.compounds.push_back((int)c); }      // (the first impact in list order has it)
        if (!im.compounds.empty()) impacts.push_back(im);
    }
    if (acted) *acted = impacts;
    if (impacts.empty()) return {};
    if (oneEvent) return ExecuteFractureRoutine(impacts, maxAxisScale, args, spherePointCloud);
    // the loop of one-impact routines: a commit erases its targets, so every compound still to come moves down by the number of
    // erased ones below it, and the compounds made so far (which sit above every old one) by all of them
    std::vector<int> made;
    std::vector<int> gone;
    // (impacts with a pattern or a flag of their own: the pattern is selected before each cycle, and the one installed now comes back)
    const bool library = std::find_if(impacts.begin(), impacts.end(), [](const Impact& im) { return im.pattern >= 0 || im.partial >= 0; }) != impacts.end();
    if (library) check_impact_patterns(impacts);
    const int installed = library ? installed_pattern_id() : -1;
    struct Reinstall { FractureEngine* e; int id; ~Reinstall() { if (id >= 0) { try { e->SelectPattern(id); } catch (const Error&) {} } } } reinstall{this, installed};
    if (library)
    {
        cell_base_.assign(1, 0u);
        for (const Impact& im : impacts)
        {
            uint32_t nc1 = 0;
            check(surtr_pattern_info(ctx_, (uint32_t)(im.pattern >= 0 ? im.pattern : installed), &nc1, nullptr), "surtr_pattern_info");
            cell_base_.push_back(cell_base_.back() + nc1);
        }
    }
    for (const Impact& im : impacts)
    {
        std::vector<int> now;
        for (int c : im.compounds) now.push_back(c - (int)std::count_if(gone.begin(), gone.end(), [c](int g) { return g < c; }));
        FractureArgs one = args;
        one.ImpactPosition = im.position; one.ImpactRadius = im.radius;
        if (library) SelectPattern(im.pattern >= 0 ? im.pattern : installed);
        if (im.partial >= 0) one.PartialFracture = im.partial != 0;
        for (int& c : made) c -= (int)now.size();
        const std::vector<int> more = ExecuteFractureRoutine(now, maxAxisScale, one, spherePointCloud);
        made.insert(made.end(), more.begin(), more.end());
        gone.insert(gone.end(), im.compounds.begin(), im.compounds.end());
    }
    return made;
}

bool ConvexRayIntersection(const VMACH::Polygon3D& convex, const Ray ray, float& dist)
{
    const double o[3] = {ray.position.x, ray.position.y, ray.position.z}, d[3] = {ray.direction.x, ray.direction.y, ray.direction.z};
    double t_in = 0.0, t_ex = DBL_MAX;
    bool any = false;
    for (const auto& f : convex.FaceVec)
    {
        if (f.VertexVec.size() < 3) continue;
        const Plane pl = f.FacePlaneConstructed ? f.FacePlane : VMACH::ConstructFacePlane(f);
        const double den = pl.x * d[0] + pl.y * d[1] + pl.z * d[2], dst = pl.x * o[0] + pl.y * o[1] + pl.z * o[2] + pl.w;
        any = true;
        if (den == 0.0) { if (dst > 0.0) return false; continue; }
        const double t = -dst / den;
        if (den < 0.0) { if (t > t_in) t_in = t; }
        else if (t < t_ex) t_ex = t;
    }
    if (!any || !(t_in <= t_ex)) return false;
    dist = (float)t_in;
    return true;
}

std::vector<surtr_mass> CompoundMass(const std::vector<std::set<int>>& bind, const std::vector<surtr_mass>& pieces)
{
    std::vector<uint32_t> off(1, 0u);
    std::vector<int32_t> members;
    for (const auto& b : bind)
    {
        for (int p : b)
        {
            if (p < 0 || (size_t)p >= pieces.size()) throw Error(SURTR_E_INVALID, "CompoundMass: piece without a record");
            members.push_back(p);
        }
        off.push_back((uint32_t)members.size());
    }
    std::vector<surtr_mass> out(bind.size());
    const int rc = bind.empty() ? SURTR_OK : surtr_combine_mass((uint32_t)bind.size(), off.data(), members.data(), pieces.data(), out.data());
    if (rc) throw Error(rc, std::string("surtr_combine_mass: ") + surtr_strerror(rc));
    return out;
}

Poly::Polyhedron FractureEngine::RefitSolid(const Poly::Polyhedron& mesh, const Poly::Polyhedron& convex)
{
    Flat m, c; m.add(mesh); c.add(convex);
    uint32_t nv = 0, nh = 0;
    const uint32_t MV = (uint32_t)mesh.size(), CV = (uint32_t)convex.size();
    check(surtr_refit_solid(ctx_, MV, m.pos.data(), m.nbr_off.data(), m.nbr.data(), CV, c.pos.data(), c.nbr_off.data(), c.nbr.data(),
                            &nv, &nh, nullptr, nullptr, nullptr), "surtr_refit_solid");
    std::vector<float> pos(3 * (size_t)nv + 3); std::vector<uint32_t> off(nv + 1); std::vector<int32_t> nbr(nh + 1);
    check(surtr_refit_solid(ctx_, MV, m.pos.data(), m.nbr_off.data(), m.nbr.data(), CV, c.pos.data(), c.nbr_off.data(), c.nbr.data(),
                            &nv, &nh, pos.data(), off.data(), nbr.data()), "surtr_refit_solid");
    return rebuild(pos.data(), off.data(), nbr.data(), 0, nv);
}

Poly::Extract FractureEngine::ExtractFaces(const Poly::Polyhedron& polyhedron)
{
    Flat in; in.add(polyhedron);
    const uint32_t V = (uint32_t)polyhedron.size();
    uint32_t nf = 0, ni = 0;
    check(surtr_extract_faces(ctx_, V, in.pos.data(), in.nbr_off.data(), in.nbr.data(), &nf, &ni, nullptr, nullptr), "surtr_extract_faces");
    std::vector<uint32_t> fo(nf + 1); std::vector<int32_t> fi(ni + 1);
    check(surtr_extract_faces(ctx_, V, in.pos.data(), in.nbr_off.data(), in.nbr.data(), &nf, &ni, fo.data(), fi.data()), "surtr_extract_faces");
    Poly::Extract out(nf);
    for (uint32_t f = 0; f < nf; ++f) out[f].assign(fi.begin() + fo[f], fi.begin() + fo[f + 1]);
    return out;
}

FragmentRender FractureEngine::RenderPolyhedron(const Poly::Polyhedron& poly, bool isConvex, const Vector3& color)
{
    Flat in; in.add(poly);
    const uint32_t V = (uint32_t)poly.size();
    const float col[3] = {color.x, color.y, color.z};
    uint32_t ni = 0;
    check(surtr_triangulate(ctx_, V, in.pos.data(), in.nbr_off.data(), in.nbr.data(), isConvex ? 1 : 0, col, nullptr, &ni, nullptr), "surtr_triangulate");
    FragmentRender r;
    r.vertexData.resize(V); r.indexData.resize(ni);
    std::vector<uint32_t> idx(ni + 1);
    check(surtr_triangulate(ctx_, V, in.pos.data(), in.nbr_off.data(), in.nbr.data(), isConvex ? 1 : 0, col, (float*)r.vertexData.data(), &ni, idx.data()),
          "surtr_triangulate");
    std::copy(idx.begin(), idx.begin() + ni, r.indexData.begin());
    return r;
}

Poly::Polyhedron FractureEngine::TransformSolid(const Poly::Polyhedron& polyhedron, const Matrix& matrix)
{
    // One lone host polyhedron: the arithmetic of k_transform (XMVector3TransformCoord(v, XMMatrixTranspose(M)): per row
    // x*m0 + (y*m1 + (z*m2 + m3)), multiply-then-add -- this file is built with -ffp-contract=off -- then the divide by w) here on
    // the host; the resident compound of this engine is not touched.  Pieces of an event are moved on the device
    // (TransformCompound).
    Poly::Polyhedron out = polyhedron;
    const float* m = matrix.m;
    for (auto& v : out)
    {
        const float x = v.Position.x, y = v.Position.y, z = v.Position.z;
        float r[4];
        for (int c = 0; c < 4; ++c)
        {
            float t = z * m[4 * c + 2] + m[4 * c + 3];
            t = y * m[4 * c + 1] + t;
            r[c] = x * m[4 * c] + t;
        }
        v.Position = Vector3(r[0] / r[3], r[1] / r[3], r[2] / r[3]);
    }
    return out;
}

// ---- the step after the event: regrouping, and DoFracture as a whole ---------------------------------------------------
bool ConvexOutOfSphere(const Poly::Polyhedron& polyhedron, const Poly::Extract* extract, const std::vector<Vector3>& spherePointCloud,
                       const Vector3 origin, const float radius)
{
    (void)extract;       // == ExtractFaces(polyhedron): derived again behind the C ABI
    Flat in; in.add(polyhedron);
    const std::vector<float> cloud = flat_points(spherePointCloud);
    const float org[3] = {origin.x, origin.y, origin.z};
    int out = 0;
    const int rc = surtr_convex_out_of_sphere((uint32_t)polyhedron.size(), in.pos.data(), in.nbr_off.data(), in.nbr.data(),
                                              (uint32_t)spherePointCloud.size(), cloud.data(), org, radius, &out);
    if (rc) throw Error(rc, std::string("ConvexOutOfSphere: ") + surtr_strerror(rc));
    return out != 0;
}

void MergeOutOfImpact(CompoundInfo& compoundInfo, const std::vector<Vector3>& spherePointCloud, const Vector3 origin, const float radius)
{
    // the set bookkeeping of Src/Surtr.cpp:2368-2403; the geometry is ConvexOutOfSphere
    for (size_t i = 1; i < compoundInfo.CompoundBind.size(); ++i)
    {
        auto& local = compoundInfo.CompoundBind[i];
        std::set<int> outside;
        for (const int c : local)
            if (ConvexOutOfSphere(compoundInfo.PieceVec[(size_t)c].Convex, nullptr, spherePointCloud, origin, radius)) outside.insert(c);
        if (!outside.empty())
        {
            for (const int c : outside) local.erase(c);
            compoundInfo.CompoundBind[0].insert(outside.begin(), outside.end());
        }
    }
    if (!compoundInfo.CompoundBind.empty())
        compoundInfo.CompoundBind.erase(std::remove_if(std::next(compoundInfo.CompoundBind.begin()), compoundInfo.CompoundBind.end(),
                                                       [](const std::set<int>& local) { return local.empty(); }),
                                        compoundInfo.CompoundBind.end());
}

void HandleConvexIsland(CompoundInfo& compoundInfo)
{
    // surtr_regroup works on pieces numbered so that compound 0 comes first and every other compound is a run of consecutive
    // pieces: renumber, regroup without the merge step, number back.  Its result order is the reference's: the first group of
    // a split compound stays where the compound was, the others are appended (Src/Surtr.cpp:2356-2365).
    auto& bind = compoundInfo.CompoundBind;
    if (bind.empty()) return;
    std::vector<int> order;                       // new index -> old piece index
    std::vector<int32_t> cell;
    for (size_t i = 0; i < bind.size(); ++i)
        for (const int c : bind[i]) { order.push_back(c); cell.push_back(i == 0 ? -1 : (int32_t)i); }
    const uint32_t n = (uint32_t)order.size(), n0 = (uint32_t)bind[0].size();
    if (n == 0) return;
    Flat cv;
    for (const int c : order) cv.add(compoundInfo.PieceVec[(size_t)c].Convex);
    std::vector<uint32_t> off(n + 2);
    std::vector<int32_t> piece(n);
    uint32_t nc = 0;
    const float org[3] = {0.f, 0.f, 0.f};
    const int rc = surtr_regroup(n, n0, cell.data(), cv.vert_off.data(), cv.pos.data(), cv.nbr_off.data(), cv.nbr.data(), 0, 0, nullptr, org, 0.f,
                                 &nc, off.data(), piece.data());
    if (rc) throw Error(rc, std::string("HandleConvexIsland: ") + surtr_strerror(rc));
    std::vector<std::set<int>> out(nc);
    for (uint32_t c = 0; c < nc; ++c)
        for (uint32_t k = off[c]; k < off[c + 1]; ++k) out[c].insert(order[(size_t)piece[k]]);
    bind.swap(out);
}

std::vector<Compound> FractureEngine::DoFracture(const Compound& targetCompound, float maxAxisScale, const FractureArgs& args,
                                                 const std::vector<Vector3>& spherePointCloud, FractureTrace* trace)
{
    // localFracturePattern (:1887), when a pair is in use
    if (pair_partial_ >= 0) SelectPattern(args.PartialFracture ? pair_partial_ : pair_general_);
    // Scale + alignment of the pattern (Src/Surtr.cpp:1890-1896): every cell scaled by MaxAxisScale * 2, moved to the impact
    const float s2 = maxAxisScale * 2.f;
    SetRefittingPointLimit(args.RefittingPointLimit);      // (before the event: its arena is sized for the refit's planes)
    PlacePattern(Vector3(s2, s2, s2), args.ImpactPosition);
    // the sphere point cloud: v *= ImpactRadius; v += ImpactPosition (:1911-1915)
    std::vector<Vector3> cloud = spherePointCloud;
    for (auto& v : cloud)
    {
        v.x *= args.ImpactRadius; v.y *= args.ImpactRadius; v.z *= args.ImpactRadius;
        v.x += args.ImpactPosition.x; v.y += args.ImpactPosition.y; v.z += args.ImpactPosition.z;
    }
    SetCompound(targetCompound);
    // ApplyFracture (:2098-2149): with PartialFracture the pieces whose Convex is out of the sphere are kept whole (bind 0)
    std::set<int> outside;
    if (args.PartialFracture)
        for (size_t c = 0; c < targetCompound.PieceVec.size(); ++c)
            if (ConvexOutOfSphere(targetCompound.PieceVec[c].Convex, nullptr, cloud, args.ImpactPosition, args.ImpactRadius)) outside.insert((int)c);
    std::vector<uint8_t> mask(n_pieces_, 0);
    for (const int o : outside) mask[(size_t)o] = 1;
    check(surtr_fracture_event(ctx_, 0, n_cells_, outside.empty() ? nullptr : mask.data(), 0u, &counts_), "surtr_fracture_event");
    std::vector<Fragment> raw;
    if (trace) raw = download_fragments(false);            // (the un-refitted Convex solids, for whoever wants to check the regrouping)
    // MergeOutOfImpact (PartialFracture) + HandleConvexIsland, on the un-refitted Convex solids where the event left them
    const std::vector<float> fc = flat_points(cloud);
    const float org[3] = {args.ImpactPosition.x, args.ImpactPosition.y, args.ImpactPosition.z};
    uint32_t np = 0, nc = 0;
    check(surtr_event_regroup(ctx_, args.PartialFracture ? 1 : 0, (uint32_t)cloud.size(), fc.data(), org, args.ImpactRadius, &np, &nc, nullptr, nullptr),
          "surtr_event_regroup");
    std::vector<uint32_t> off(np + 2);
    std::vector<int32_t> piece(np + 1);
    check(surtr_event_regroup(ctx_, args.PartialFracture ? 1 : 0, (uint32_t)cloud.size(), fc.data(), org, args.ImpactRadius, &np, &nc, off.data(), piece.data()),
          "surtr_event_regroup");
    // Refitting (:1937-1939), then the pieces: the skipped ones first (ascending), then the fragments in output order
    check(surtr_event_refit(ctx_), "surtr_event_refit");
    check(surtr_event_counts(ctx_, &counts_), "surtr_event_counts");
    const std::vector<Fragment> frags = download_fragments(false);
    report_flagged(frags, 0, n_cells_, "DoFracture");
    const uint32_t n0 = (uint32_t)outside.size();
    if (np != n0 + frags.size()) throw Error(SURTR_E_STATE, "DoFracture: piece count of the regrouping does not match the event");
    std::vector<const Piece*> all;
    for (const int o : outside) all.push_back(&targetCompound.PieceVec[(size_t)o]);
    for (const auto& f : frags) all.push_back(&f.piece_data);
    std::vector<Compound> result(nc);
    for (uint32_t c = 0; c < nc; ++c)
        for (uint32_t k = off[c]; k < off[c + 1]; ++k) result[c].PieceVec.push_back(*all[(size_t)piece[k]]);
    if (trace)
    {
        trace->nOutside = n0; trace->Convex.clear(); trace->PieceCell.clear(); trace->CompoundBind.assign(nc, {});
        for (const int o : outside) { trace->Convex.push_back(targetCompound.PieceVec[(size_t)o].Convex); trace->PieceCell.push_back(-1); }
        for (const auto& f : raw) { trace->Convex.push_back(f.piece_data.Convex); trace->PieceCell.push_back(f.cell); }
        for (uint32_t c = 0; c < nc; ++c) for (uint32_t k = off[c]; k < off[c + 1]; ++k) trace->CompoundBind[c].insert(piece[k]);
    }
    return result;
}

// ---- the per-Piece tasks with the reference's signatures (Inc/Surtr.h:270-272) --------------------------------------------
std::vector<Piece*> FractureTask(const VMACH::Polygon3D& voroPoly, const std::vector<Piece*>& targetPieceVec, const std::set<int>& outside)
{
    // m_fractureTask (Src/Surtr.cpp:1457-1504) for one cell: clip Convex, then Mesh, split islands; no refit here
    FractureEngine& eng = DefaultEngine();
    Compound comp;
    for (const Piece* p : targetPieceVec) comp.PieceVec.push_back(*p);
    eng.SetPattern(std::vector<VMACH::Polygon3D>{voroPoly});
    eng.PlacePattern(Vector3(1.f, 1.f, 1.f), Vector3(0.f, 0.f, 0.f));      // the cell comes placed: x * 1 + 0 leaves every float as it is
    eng.SetCompound(comp);
    const std::vector<Fragment> frags = eng.ApplyFracture(outside, false, false);
    std::vector<Piece*> out;
    for (const auto& f : frags) out.push_back(new Piece(f.piece_data.Convex, f.piece_data.Mesh));
    return out;
}

void RefittingTask(Piece* piece)
{
    // m_refittingTask (Src/Surtr.cpp:1449-1455), at the default engine's RefittingPointLimit
    piece->Convex = DefaultEngine().RefitSolid(piece->Mesh, piece->Convex);
}

InitCompoundResult InitCompoundTask(const Piece* piece, const Poly::Extract* extract, bool renderConvex)
{
    // m_initCompoundTask (Src/Surtr.cpp:1436-1447): the points PxCreateConvexMesh cooks (:2531-2553) and the buffers
    // DynamicMesh::UpdateMeshData uploads -- RenderPolyhedron of the Convex (as convex) or of the Mesh (isConvex = false)
    (void)extract;
    InitCompoundResult r;
    for (const auto& v : piece->Convex) r.ConvexPoints.push_back(v.Position);
    r.Mesh = DefaultEngine().RenderPolyhedron(renderConvex ? piece->Convex : piece->Mesh, renderConvex, Vector3(0.25f, 0.25f, 0.25f));
    if (DefaultEngine().RenderNormals())      // (RenderPolyhedron left the solid as the engine's only fragment, triangulated: the same device call)
    {
        std::vector<surtr_shaded> rec;
        r.MeshLit = std::move(DefaultEngine().ShadedRender(Vector3(0.25f, 0.25f, 0.25f), &rec).front());
        r.Lit = rec.front();
    }
    return r;
}

} // namespace surtr
