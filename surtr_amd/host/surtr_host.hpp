// surtr_host.hpp -- C++ host layer that keeps the reference's type and function names for the
// fracture-event path (Inc/Poly.h:15-76, Inc/Kdop.h:16-41, Inc/VMACH.h:17-86, Inc/Surtr.h:113-134, 270-272) and
// forwards the work to the HIP engine through the C ABI of include/surtr_hip.h.
//
// It is what a front-end (the DX12 demo or a headless harness) links instead of Src/Poly.cpp / Src/Kdop.cpp and the
// hot-path members of Src/Surtr.cpp.  No geometry is computed here: the types are thin views that are flattened to CSR
// buffers, sent through the C ABI and rebuilt from the result.  The free functions of namespace Poly / Kdop keep the
// reference's signatures; they run on a process-wide default engine (DefaultEngine()).
#pragma once
#include <cfloat>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <set>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../include/surtr_hip.h"

namespace surtr {

struct Vector3 { float x = 0, y = 0, z = 0; Vector3() = default; Vector3(float a, float b, float c) : x(a), y(b), z(c) {} };
struct Plane { float x = 0, y = 0, z = 0, w = 0; Plane() = default; Plane(float a, float b, float c, float d) : x(a), y(b), z(c), w(d) {} };
// DirectX::XMMATRIX as the reference stores it in m_structuredBufferData[i].WorldMatrix (row-major, 16 floats).
struct Matrix { float m[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}; };

// The reference throws std::exception (Src/Poly.cpp:258); the C ABI returns codes; this layer rethrows.
struct Error : std::runtime_error
{
    int code;
    Error(int c, const std::string& what) : std::runtime_error(what), code(c) {}
};

// VertexNormalColor, Inc/Mesh.h:4-13: three XMFLOAT3, 36 bytes, what DynamicMesh::UploadVB copies into the D3D12 upload
// heap (Inc/Mesh.h:163-183).  The engine's `vnc` buffers have exactly this layout.
struct VertexNormalColor { float Position[3]; float Normal[3]; float Color[3]; };
static_assert(sizeof(VertexNormalColor) == 36, "VertexNormalColor is three packed XMFLOAT3 (Inc/Mesh.h:4-13)");
static_assert(offsetof(VertexNormalColor, Position) == 0 && offsetof(VertexNormalColor, Normal) == 12 && offsetof(VertexNormalColor, Color) == 24,
              "field offsets of Inc/Mesh.h:4-13");
static_assert(sizeof(Vector3) == 12, "Vector3 = XMFLOAT3: a Convex's positions are a stride-12 PxConvexMeshDesc::points array (Src/Surtr.cpp:2531-2553)");

class FractureEngine;
// Engine behind the free functions below (created on first use on device `SetDefaultDevice`, default 0).
FractureEngine& DefaultEngine();
void SetDefaultDevice(int device);

namespace VMACH {
// Inc/VMACH.h:17-58, the members the path reads and the ones that keep FacePlane current.
struct PolygonFace
{
    bool GuaranteeConvex = true;
    std::vector<Vector3> VertexVec;
    Plane FacePlane;
    bool FacePlaneConstructed = false;
    PolygonFace() = default;
    explicit PolygonFace(bool guaranteeConvex) : GuaranteeConvex(guaranteeConvex) {}
    PolygonFace(bool guaranteeConvex, std::vector<Vector3> vertexVec) : GuaranteeConvex(guaranteeConvex), VertexVec(std::move(vertexVec)) { ConstructFacePlane(); }
    void AddVertex(const Vector3& newVertex);          // Src/VMACH.cpp:289-300 (exact duplicates are dropped)
    void ConstructFacePlane();                         // Src/VMACH.cpp:302-310: Plane(V0, V1, V2), normalised
    Vector3 GetNormal() const;                         // Src/VMACH.cpp:88-97 (throws if the plane was never built)
};
struct Polygon3D                                       // Inc/VMACH.h:60-86
{
    bool GuaranteeConvex = true;
    std::vector<PolygonFace> FaceVec;
    Polygon3D() = default;
    explicit Polygon3D(bool guaranteeConvex) : GuaranteeConvex(guaranteeConvex) {}
    void AddFace(const PolygonFace& newFace) { FaceVec.push_back(newFace); }
    void Translate(const Vector3& vector);             // Src/VMACH.cpp:506-514 (+ ConstructFacePlane)
    void Scale(const Vector3& vector);                 // Src/VMACH.cpp:525-534
};
Plane ConstructFacePlane(const PolygonFace& f);
} // namespace VMACH

namespace Poly {
struct Vertex                                   // Inc/Poly.h:15-30
{
    Vector3 Position;
    std::vector<int> NeighborVertexVec;
    int comp = 1;
    mutable int ID = -1;
};
typedef std::vector<Vertex> Polyhedron;         // Inc/Poly.h:31
typedef std::vector<std::vector<int>> Extract;  // Inc/Poly.h:32

// Inc/Poly.h:35-76, same names and argument meaning.
void InitPolyhedron(Polyhedron& polyhedron, const std::vector<Vector3>& positionVec, const std::vector<std::vector<int>>& neighborVec);
void Moments(double& zerothMoment, Vector3& firstMoment, const Polyhedron& polyhedron);          // Src/Poly.cpp:55-87
Extract* ExtractFaces(const Polyhedron& polyhedron);                                              // Src/Poly.cpp:89-126 (caller owns)
std::vector<std::vector<int>> ExtractNeighborFromMesh(std::vector<Vector3>& vertices, std::vector<int>& indices);   // Src/Poly.cpp:128-263
void ClipPolyhedron(Polyhedron& polyhedron, const std::vector<Plane>& planes);                    // Src/Poly.cpp:265-554
Polyhedron ClipPolyhedron(const Polyhedron& polyhedron, const VMACH::Polygon3D& polygon3D);       // Src/Poly.cpp:556-566
void Translate(Polyhedron& polyhedron, const Vector3& v);
void Scale(Polyhedron& polyhedron, const Vector3& v);
void Transform(Polyhedron& polyhedron, const Matrix& matrix);                                     // Src/Poly.cpp:580-585
Polyhedron GetBB();                                                                               // Src/Poly.cpp:587-617
// Src/Poly.cpp:681-714.  `extract` must be ExtractFaces(poly) (the kernels derive the faces themselves); vertices and
// indices are appended after what the two vectors hold, indices offset by the vertices already there, as in the reference.
void RenderPolyhedron(std::vector<VertexNormalColor>& vertexData, std::vector<uint32_t>& indexData, const Polyhedron& poly,
                      const Extract* extract, bool isConvex = true, Vector3 color = Vector3(0.25f, 0.25f, 0.25f));
// Inc/Poly.h:50-61, Src/Poly.cpp:619-679: three unshared vertices per triangle, each with the normal of its face, and running indices
// (offset by the vertices already there, as above).  The normals are those of include/surtr_hip.h, "lit render buffers" (the Newell sum of
// the whole loop; the reference takes the first three vertices); the triangles are RenderPolyhedron's for the same isConvex.
void RenderPolyhedronNormal(std::vector<VertexNormalColor>& vertexData, std::vector<uint32_t>& indexData, const Polyhedron& poly, bool isConvex,
                            Vector3 color = Vector3(0.25f, 0.25f, 0.25f));
void RenderPolyhedronNormal(std::vector<VertexNormalColor>& vertexData, std::vector<uint32_t>& indexData, const Polyhedron& poly,
                            const Extract* extract, bool isConvex, Vector3 color = Vector3(0.25f, 0.25f, 0.25f));
} // namespace Poly

namespace Kdop {
struct KdopElement                              // Inc/Kdop.h:16-27
{
    Vector3 Normal, MinVertex, MaxVertex;
    double MinDist = DBL_MAX, MaxDist = -DBL_MAX;
    Plane MinPlane, MaxPlane;
    explicit KdopElement(const Vector3& normal) : Normal(normal) {}
};
struct KdopContainer                            // Inc/Kdop.h:29-41
{
    std::vector<KdopElement> ElementVec;
    explicit KdopContainer(const std::vector<Vector3>& normalVec);                                          // Src/Kdop.cpp:10-13
    void Calc(const std::vector<Vector3>& vertices, const double& maxAxisScale, const float& planeGapInv);   // Src/Kdop.cpp:15-51
    void Calc(const Poly::Polyhedron& mesh);                                                                // Src/Kdop.cpp:92-115
    Poly::Polyhedron ClipWithPolyhedron(const Poly::Polyhedron& polyhedron);                                // Src/Kdop.cpp:166-179
};
} // namespace Kdop

// Surtr::GenerateICHNormal (Src/Surtr.cpp:1961-1982): unit face normals of VMACH::ConvexHull(vertices, limitCnt).
std::vector<Vector3> GenerateICHNormal(const std::vector<Vector3>& vertices, int limitCnt);

// Surtr::LoadModelData (Src/Surtr.cpp:2683-2727) for Wavefront OBJ: positions with x negated, scaled, translated; triangles
// with the winding flipped; identical positions joined (normals are not read: the path does not use them).
void LoadModelData(const std::string& fileName, const Vector3& scale, const Vector3& translate, std::vector<Vector3>& vertices,
                   std::vector<int>& indices);

struct Piece                                                // Inc/Surtr.h:113-119 (the reference heap-allocates them: Piece*)
{
    Poly::Polyhedron Convex, Mesh;
    Piece() = default;
    Piece(const Poly::Polyhedron& convex, const Poly::Polyhedron& mesh) : Convex(convex), Mesh(mesh) {}
};
struct Compound { std::vector<Piece> PieceVec; };           // Inc/Surtr.h:121-127 (value semantics: no leaks)
// Inc/Surtr.h:129-134: pieces + bind sets (CompoundBind[0] = the pieces outside the impact).
struct CompoundInfo { std::vector<Piece> PieceVec; std::vector<std::set<int>> CompoundBind; };

// Surtr::FractureArgs, the members the event reads (Inc/Surtr.h:90-110; Src/Surtr.cpp:1885-1912).
struct FractureArgs
{
    bool PartialFracture = false;
    Vector3 ImpactPosition;
    float ImpactRadius = 1.f;
    int Seed = 46354;
    int RefittingPointLimit = 4;      // points of the limited hull behind a fragment's slab planes (Inc/Surtr.h:93): 4 .. 32 here
    bool RadialMode = true;           // Inc/Surtr.h:100: an impact takes every body its sphere touches, not only the one hit
    float TargetAdder = 0.01f;        // Inc/Surtr.h:109: how far behind the hit the impact is placed, along the ray
    // the two resident fracture patterns (Inc/Surtr.h:102-107; built at Src/Surtr.cpp:1806-1807): PrepareFracturePatterns
    float PartialFracturePatternDist = 0.01f;
    float GeneralFracturePatternDist = 1.0f;
    int PartialFracturePatternCellCnt = 128;
    int GeneralFracturePatternCellCnt = 1024;
    // the cooker's tolerances, absolute, as CookingConvex sets them (Src/Surtr.cpp:2531-2553: eWELD_VERTICES with no weld distance,
    // planeTolerance 0.000007f): FractureEngine::CookHulls / CookPieceHulls / InitCompounds(..., cookUnusable)
    float CookWeldDistance = 0.f;
    float CookPlaneTolerance = 7e-6f;
    float HullRelTolerance = 1e-5f;   // HullUsable's relTol: which pieces the cooker takes
};

// DirectX::SimpleMath::Ray as OnMouseDown builds it (Src/Surtr.cpp:178-200): the direction is expected to be of unit length.
// One contact of a frame above the report threshold: where, how large, and the compounds it breaks.
// pattern: the stored pattern (FractureEngine::StorePattern) its cells come from, -1 the engine's installed pattern; partial: 0 / 1
// FractureArgs::PartialFracture for this impact alone, -1 what the call's args say.  Left at -1, both mean what they meant before.
struct Impact { Vector3 position; float radius = 0.f; std::vector<int> compounds; int pattern = -1; int partial = -1; };
// One Impact per pair of bodies the contacts name, in record order of the pair's first record: at the midpoint of the witness points
// of that pair's closest record (ties: the first in record order), of the radius given, naming both bodies.  Ready for OnImpacts.
std::vector<Impact> ImpactsFromContacts(const std::vector<surtr_contact>& contacts, float radius);
struct Ray { Vector3 position, direction; Ray() = default; Ray(const Vector3& p, const Vector3& d) : position(p), direction(d) {} };
// Surtr::ConvexRayIntersection (Src/Surtr.cpp:2460-2497), on the host from the definition of include/surtr_hip.h: the ray's
// interval [0, inf) clipped by the half-space of every face plane (FacePlane; built from the first three vertices where it was
// never constructed).  True when something is left; dist = the entry parameter (0 from inside).
bool ConvexRayIntersection(const VMACH::Polygon3D& convex, const Ray ray, float& dist);

struct FragmentRender { std::vector<VertexNormalColor> vertexData; std::vector<uint32_t> indexData; };

// Surtr::ConvexOutOfSphere (Src/Surtr.cpp:2415-2458); `extract` = ExtractFaces(polyhedron) (derived again inside).
bool ConvexOutOfSphere(const Poly::Polyhedron& polyhedron, const Poly::Extract* extract, const std::vector<Vector3>& spherePointCloud,
                       const Vector3 origin, const float radius);
// Surtr::MergeOutOfImpact (Src/Surtr.cpp:2368-2403): pieces of the compounds 1.. that are out of the sphere move to compound 0;
// compounds left empty are removed.
void MergeOutOfImpact(CompoundInfo& compoundInfo, const std::vector<Vector3>& spherePointCloud, const Vector3 origin, const float radius);
// Surtr::HandleConvexIsland (Src/Surtr.cpp:2203-2366): every compound is split into the groups of pieces that touch through a
// pair of opposite, overlapping faces; the first group stays, the others are appended.
void HandleConvexIsland(CompoundInfo& compoundInfo);

// The three per-Piece tasks with the reference's EXACT signatures (Inc/Surtr.h:270-272: pointer semantics; what they return is
// the caller's, as Src/Surtr.cpp:1494,1499 `new Piece`), on the default engine.  m_initCompoundTask's result pair
// <PxConvexMeshGeometry, DynamicMesh*> needs PhysX and D3D12: InitCompoundResult holds what those two are built from.
std::vector<Piece*> FractureTask(const VMACH::Polygon3D& voroPoly, const std::vector<Piece*>& targetPieceVec, const std::set<int>& outside);
void RefittingTask(Piece* piece);
// Hull (filled only when asked for, withHulls): what CookingConvexManual (Src/Surtr.cpp:2555-2614) takes from
// Compound::PieceExtractedConvex -- the Convex's face loops as PxHullPolygon records with 16-bit indices into ConvexPoints, the planes
// as include/surtr_hip.h defines them, and the record that says whether the hull can skip quickhull (HullUsable).
struct HullData { surtr_hull Record{}; std::vector<surtr_hull_polygon> Polygons; std::vector<uint16_t> Indices; };
// Cooked (filled only with cookUnusable, and only for a piece HullUsable refuses; else Record.status == SURTR_COOK_SKIPPED): the
// convex hull of ConvexPoints built on the device (include/surtr_hip.h, "cooked hulls") -- Points / Polygons / Indices go into
// PxConvexMeshDesc as they are (16-bit indices), Source names the ConvexPoints entry of every point.
struct CookedData
{
    surtr_cooked Record{}; std::vector<Vector3> Points; std::vector<uint32_t> Source; std::vector<surtr_hull_polygon> Polygons; std::vector<uint16_t> Indices;
};
// MeshLit / Lit (filled only under FractureEngine::SetRenderNormals(true)): the lit buffers of the same solid and triangles as Mesh --
// one vertex per index, running indices -- and the piece's record (faces, SURTR_SHADE_PER_TRIANGLE).
struct InitCompoundResult { std::vector<Vector3> ConvexPoints; FragmentRender Mesh; HullData Hull; CookedData Cooked; FragmentRender MeshLit; surtr_shaded Lit{}; };
// No withholding bit, planarity within planeTol and convexity within 2 planeTol + weldDist, each plus the rounding of a written
// plane at its largest: 2^-24 * 3.5 * reach (|n_x| + |n_y| + |n_z| <= sqrt 3, |d| <= sqrt 3 * reach).  A cooked hull that fails --
// a flat or otherwise withheld solid -- is left to PxConvexFlag::eCOMPUTE_CONVEX.
inline bool CookedUsable(const surtr_cooked& c, float planeTol = 7e-6f, float weldDist = 0.f)
{
    if (c.status & ~(uint32_t)SURTR_COOK_OVER_255) return false;
    const double s = 3.5 * (double)c.reach / 16777216.0;
    return (double)c.planarity <= (double)planeTol + s && (double)c.convexity <= 2.0 * (double)planeTol + (double)weldDist + s;
}
// The cooked hulls of a set of solids as the device wrote them: Records[k]'s points are Points[3 pt_off ..) (and Source[pt_off ..)),
// its polygons Polygons[face_off ..), its indices Indices[idx_off ..), solid-local.
struct CookedSet
{
    std::vector<surtr_cooked> Records; std::vector<float> Points; std::vector<uint32_t> Source; std::vector<surtr_hull_polygon> Polygons;
    std::vector<uint16_t> Indices;
};
// No withholding bit, no flat face, and both errors within relTol of the solid's extent.  A hull that fails falls back to
// ConvexPoints (PxConvexFlag::eCOMPUTE_CONVEX, CookingConvex :2531-2553).
inline bool HullUsable(const surtr_hull& h, float relTol = 1e-5f)
{
    if (h.status & (SURTR_HULL_FEW | SURTR_HULL_OPEN | SURTR_HULL_IRREGULAR | SURTR_HULL_LARGE | SURTR_HULL_FLAT)) return false;
    const float tol = relTol * h.extent;
    return h.convexity <= tol && h.planarity <= tol;
}
// The hulls of a set of solids as the device wrote them: Records[k]'s polygons are Polygons[face_off .. face_off + n_faces), its
// indices Indices[idx_off .. idx_off + n_idx), solid-local.
struct HullSet { std::vector<surtr_hull> Records; std::vector<surtr_hull_polygon> Polygons; std::vector<uint16_t> Indices; };
InitCompoundResult InitCompoundTask(const Piece* piece, const Poly::Extract* extract, bool renderConvex);

struct Fragment { int cell, piece, island; Piece piece_data; FragmentRender render; int status = 0; };

// One engine per GPU (wraps surtr_ctx).  Mirrors the calls of Surtr::DoFracture (Src/Surtr.cpp:1885-1959).
// The records of compounds from the records of their pieces (surtr_combine_mass: parallel-axis theorem, host).  bind = the
// bind sets of surtr_event_regroup / FractureTrace::CompoundBind; pieces numbered as there.
std::vector<surtr_mass> CompoundMass(const std::vector<std::set<int>>& bind, const std::vector<surtr_mass>& pieces);

class FractureEngine
{
public:
    explicit FractureEngine(int device = 0);
    ~FractureEngine();
    FractureEngine(const FractureEngine&) = delete;
    FractureEngine& operator=(const FractureEngine&) = delete;

    // Fracture pattern in pattern space (GenerateFracturePattern / GenerateVoronoi, Src/Surtr.cpp:2003-2096).
    void SetPattern(const std::vector<VMACH::Polygon3D>& voroPolyVec);
    // Surtr::GenerateVoronoi(cellPointVec) (Src/Surtr.cpp:2003-2070; voro++ replaced by the canonical cell of DESIGN section 5)
    // ON THE DEVICE: surtr_build_cells, which also installs the cells as this engine's pattern, + surtr_download_cells.
    std::vector<VMACH::Polygon3D> GenerateVoronoi(const std::vector<Vector3>& cellPointVec);
    // Surtr::GenerateVoronoi(cellCnt) (Src/Surtr.cpp:1984-2001): mt19937(seed), uniform(-0.5, 0.5) in x, y, z draw order.
    std::vector<VMACH::Polygon3D> GenerateVoronoi(int cellCnt, int seed = 46354);
    // Surtr::GenerateFracturePattern (Src/Surtr.cpp:2072-2096): exponential length (clamped to [1e-12, 0.5]) x normalised
    // uniform(-1, 1)^3 direction.
    std::vector<VMACH::Polygon3D> GenerateFracturePattern(int cellCount, double mean, int seed = 46354);
    // the same cells from the host builder (surtr_voronoi_cells): the CPU-tier cross-check of the device builder
    static std::vector<VMACH::Polygon3D> GenerateVoronoiHost(const std::vector<Vector3>& cellPointVec);
    // voro.Scale(scale); voro.Translate(translate) for every cell (Src/Surtr.cpp:1799-1803, 1891-1896).
    void PlacePattern(const Vector3& scale, const Vector3& translate);
    // ---- the pattern library (surtr_pattern_store / _select / _count / _clear): several patterns resident on the device ----
    // StorePattern: the installed pattern (SetPattern / GenerateVoronoi / GenerateFracturePattern / SelectPattern) into the library
    // -> its id.  SelectPattern: a stored pattern becomes the installed one, device to device.  ClearPatterns drops all of them.
    int StorePattern();
    void SelectPattern(int id);
    int PatternCount();
    void ClearPatterns();
    // The two patterns the reference keeps for the session (Src/Surtr.cpp:1806-1807), built and stored in its order: the partial one
    // (PartialFracturePatternCellCnt cells at mean PartialFracturePatternDist), then the general one -> {partialId, generalId}.  The
    // general pattern is the installed one afterwards.
    std::pair<int, int> PrepareFracturePatterns(const FractureArgs& args);
    // After this DoFracture selects by args.PartialFracture as :1887 does: the partial pattern when it is set, else the general
    // one.  (-1, -1): DoFracture uses the installed pattern again, as it does when this was never called.
    void UsePatternPair(int partialId, int generalId);
    void SetCompound(const Compound& compound);
    // ExecuteFractureRoutine's pre-transform (Src/Surtr.cpp:1846-1851): Poly::Transform of every resident piece's Convex and
    // Mesh by its world matrix, on the device.
    void TransformCompound(const std::vector<Matrix>& worldMatrices);
    // ApplyFracture + Refitting + per-piece ExtractFaces/RenderPolyhedron (Src/Surtr.cpp:2098-2149, 2405-2413, 1436-1447):
    // fragments in cell-major, piece, island order.
    std::vector<Fragment> ApplyFracture(const std::set<int>& outside = {}, bool refit = true, bool render = true,
                                        uint32_t cellBegin = 0, uint32_t cellEnd = 0xFFFFFFFFu);
    // Recursive refracture: the fragments of the last ApplyFracture (all, or those with keep[k] != 0) become the compound of
    // the next one without leaving the device.  Returns the number of pieces.
    uint32_t CompoundFromLastEvent(const std::vector<uint8_t>& keep = {});
    // Surtr::Refitting (Src/Surtr.cpp:2405-2413): m_refittingTask on every piece.
    void Refitting(std::vector<Piece>& pieceVec);
    // Steps 1-6 of Surtr::PrepareFracture (Src/Surtr.cpp:1750-1785): ICH(limit) face normals -> k-DOP slabs moved out by
    // MaxAxisScale / planeGapInverse -> the 2x bounding box clipped by all of them (the approximate convex hull).
    Poly::Polyhedron BuildACH(const std::vector<Vector3>& vertices, uint32_t ichIncludePointLimit = 20, float achPlaneGapInverse = 2000.f);
    // Surtr::PrepareFracture (Src/Surtr.cpp:1747-1827) from a raw triangle mesh: ACH, neighbour rings, `cellCnt` Voronoi cells
    // placed over the bounding box, one event with refit + extraction.  Returns the pieces of the initial compound.
    std::vector<Fragment> PrepareFracture(std::vector<Vector3>& vertices, std::vector<int>& indices, const std::vector<Vector3>& cellPointVec);
    // Poly::ClipPolyhedron(polyhedron, polygon3D), Src/Poly.cpp:556-566.
    Poly::Polyhedron ClipPolyhedron(const Poly::Polyhedron& polyhedron, const VMACH::Polygon3D& polygon3D);
    Poly::Polyhedron ClipPolyhedron(const Poly::Polyhedron& polyhedron, const std::vector<Plane>& planes);
    // The per-Piece tasks on one solid (m_refittingTask, Poly::ExtractFaces, Poly::RenderPolyhedron, Poly::Transform).
    Poly::Polyhedron RefitSolid(const Poly::Polyhedron& mesh, const Poly::Polyhedron& convex);
    Poly::Extract ExtractFaces(const Poly::Polyhedron& polyhedron);
    FragmentRender RenderPolyhedron(const Poly::Polyhedron& poly, bool isConvex, const Vector3& color);
    Poly::Polyhedron TransformSolid(const Poly::Polyhedron& polyhedron, const Matrix& matrix);
    // Poly::RenderPolyhedronNormal on one solid: surtr_triangulate presents and triangulates it, surtr_event_shaded lights it.
    FragmentRender RenderPolyhedronNormal(const Poly::Polyhedron& poly, bool isConvex, const Vector3& color);
    // The lit buffers of every current fragment (surtr_event_shaded), one FragmentRender each with indices 0, 1, 2, ...; valid wherever
    // Hulls() is, once the fragments are triangulated (ApplyFracture with render, InitCompounds).  records: the per-fragment records.
    std::vector<FragmentRender> ShadedRender(const Vector3& color = Vector3(0.25f, 0.25f, 0.25f), std::vector<surtr_shaded>* records = nullptr);
    // On: InitCompound(s) and InitCompoundTask fill InitCompoundResult::MeshLit / Lit from the same device call.  Off (the default):
    // every result is byte for byte what it is without this switch.
    void SetRenderNormals(bool on) { render_normals_ = on; }
    bool RenderNormals() const { return render_normals_; }
    // What DoFracture regrouped (for tests and tools): the un-refitted Convex solids in piece order (the compound's pieces the
    // event skipped, ascending, then the event's fragments), the cell of every piece (-1: skipped), the bind sets found.
    struct FractureTrace { std::vector<Poly::Polyhedron> Convex; std::vector<int> PieceCell; uint32_t nOutside = 0; std::vector<std::set<int>> CompoundBind; };
    // Surtr::DoFracture (Src/Surtr.cpp:1885-1959) on the device, in the reference's order: pattern scaled by 2 * maxAxisScale
    // and moved to the impact, sphere cloud scaled by the radius and moved to the impact, ApplyFracture (pieces out of the
    // sphere are skipped when PartialFracture), MergeOutOfImpact (when PartialFracture), HandleConvexIsland -- both on the
    // un-refitted Convex solids, surtr_event_regroup --, Refitting (surtr_event_refit), one Compound per bind set.  The
    // pattern is the engine's (SetPattern / GenerateVoronoi / GenerateFracturePattern), in pattern space.
    std::vector<Compound> DoFracture(const Compound& targetCompound, float maxAxisScale, const FractureArgs& args,
                                     const std::vector<Vector3>& spherePointCloud, FractureTrace* trace = nullptr);
    // PxRigidBodyExt::updateMassAndInertia(body, 10.0f) of InitCompound (Src/Surtr.cpp:2520) without PhysX: volume, mass,
    // centre of mass and inertia tensor of every fragment of the last event (set 0 = Mesh, 1 = Convex), on the device
    // (surtr_event_mass; definition in include/surtr_hip.h).  PieceMassProperties: the same for the resident pieces.
    // Face loops and planes of the Convex of every current fragment / resident piece, on the device (surtr_event_hulls /
    // surtr_pieces_hulls; definition in include/surtr_hip.h).  SetExtract (Src/Surtr.cpp:2151-2155): the same loops of the current
    // fragments as Compound::PieceExtractedConvex holds them, from the same download.
    HullSet Hulls();
    HullSet PieceHulls();
    // Cooked hulls (surtr_event_cook / surtr_pieces_cook) of the current fragments / the resident pieces.  unusableOnly: only the
    // solids whose ring hull HullUsable refuses at relTol are cooked (the rest come back SURTR_COOK_SKIPPED); else every solid.
    CookedSet CookHulls(bool unusableOnly = true, float relTol = 1e-5f, float weldDistance = 0.f, float planeTolerance = 7e-6f);
    CookedSet CookPieceHulls(bool unusableOnly = true, float relTol = 1e-5f, float weldDistance = 0.f, float planeTolerance = 7e-6f);
    std::vector<Poly::Extract> SetExtract();
    std::vector<surtr_mass> MassProperties(int set, float density = 10.f);
    std::vector<surtr_mass> PieceMassProperties(int set, float density = 10.f);
    // OnMouseDown's scene queries (Src/Surtr.cpp:207-240) on the Convex solids of the resident pieces, on the device
    // (surtr_pieces_raycast / surtr_pieces_overlap; definition in include/surtr_hip.h).  OverlapSphere: one value per resident
    // piece, 0 not touched, 1 touched, 2 touched but of mass <= minMass (density 10, as InitCompound; minMass < 0: no gate).
    surtr_ray_hit Raycast(const Vector3& origin, const Vector3& dir, float maxDist = 1000.f);
    std::vector<uint8_t> OverlapSphere(const Vector3& centre, float radius, float minMass = 1e-4f);
    // What OnMouseDown does with them: a hit sets args.ImpactPosition = hit + dir * args.TargetAdder and returns the compounds
    // affected, ascending -- with args.RadialMode those of the pieces a sphere of radius args.ImpactRadius / 2 about the impact
    // touches and whose mass is above 1e-4 (Src/Surtr.cpp:228), else the compound of the piece hit.  pieceCompound[p] = compound of
    // resident piece p.  No hit: nothing is returned and args is left as it was.
    std::vector<int> PickImpact(const Vector3& origin, const Vector3& dir, FractureArgs& args, const std::vector<int>& pieceCompound);
    // ---- the click loop on a resident scene (OnMouseDown, Src/Surtr.cpp:178-254; ExecuteFractureRoutine, :1829-1883) ----
    // FractureStorage::CompoundVec on the device: the pieces of all compounds become resident, compound c a contiguous range of
    // them in the order of m_structuredBufferData (:1840-1843).  SceneCompounds: c owns pieces [off[c], off[c + 1]).
    void SetScene(const std::vector<Compound>& compoundVec);
    std::vector<uint32_t> SceneCompounds();
    // ExecuteFractureRoutine for one compound of the scene, in its order: Poly::Transform of that compound's pieces by `world`
    // (one matrix per piece; empty: the compound's stored pose is baked in, ApplyPose -- nothing with the identity), the pattern scaled by 2 * maxAxisScale and moved to
    // the impact, the event on that compound (with PartialFracture its pieces out of the sphere are skipped: their Convex solids,
    // a few dozen vertices each, are read back for ConvexOutOfSphere -- nothing else leaves the device), the regrouping, the refit,
    // and the commit: the compound is erased, what it broke into is pushed to the back.  Returns the numbers of the new compounds.
    // A flagged fragment is left out of the scene: as everywhere, that throws unless AllowFlagged(true).
    std::vector<int> ExecuteFractureRoutine(int compound, const std::vector<Matrix>& world, float maxAxisScale, const FractureArgs& args,
                                            const std::vector<Vector3>& spherePointCloud);
    // ExecuteFractureRoutine for every compound a click hit, in ONE pass (surtr_scene_fracture_bodies): the compounds may come in any
    // order; they are sorted descending, a duplicate throws Error(SURTR_E_INVALID).  In order: ApplyPoses, the placement, the device
    // out-of-sphere mask when PartialFracture (OutsideMask: nothing is read back but the bytes), one event over all of them, one
    // regrouping, one refit, one commit.  Returns the compounds made: the scene is the one the one-compound routine called per
    // compound in descending number leaves.  One difference: when the event flagged a unit and AllowFlagged is off, NOTHING of the
    // click is committed, where the one-compound route has committed the compounds it had dealt with before it threw.
    std::vector<int> ExecuteFractureRoutine(const std::vector<int>& compounds, float maxAxisScale, const FractureArgs& args,
                                            const std::vector<Vector3>& spherePointCloud);
    // Surtr::ConvexOutOfSphere of every piece of the listed compounds, on the device (surtr_scene_outside): one byte per piece,
    // compound after compound in the order given.  cloud: the sphere's points as placed (scaled by the radius, moved to the impact).
    std::vector<uint8_t> OutsideMask(const std::vector<int>& compounds, const FractureArgs& args, const std::vector<Vector3>& cloud);
    // PickImpact with the scene's own table.
    std::vector<int> PickImpact(const Vector3& origin, const Vector3& dir, FractureArgs& args);
    // OnMouseDown: PickImpact, then ExecuteFractureRoutine for every compound hit in DESCENDING number, so that the numbers of
    // the compounds still to come stay valid (the reference holds pointers there).  Returns the new compounds as numbered after
    // the last commit; hitCompounds (may be null) receives what PickImpact returned.
    // oneEvent: every compound hit goes through the several-compound ExecuteFractureRoutine instead (one event, one regrouping, one commit).
    std::vector<int> OnMouseDown(const Vector3& origin, const Vector3& dir, FractureArgs& args, float maxAxisScale,
                                 const std::vector<Vector3>& spherePointCloud, std::vector<int>* hitCompounds = nullptr, bool oneEvent = false);
    // InitCompound (Src/Surtr.cpp:2499-2529) for bodies of the resident scene: per piece of the body, in piece order, what
    // m_initCompoundTask (:1436-1447) hands to PxCreateConvexMesh (ConvexPoints) and to DynamicMesh (Mesh = RenderPolyhedron of the Mesh,
    // or of the Convex as convex with renderConvex), in the resident frame.  One device call (surtr_scene_fragments: nothing is read
    // back to triangulate) and one download for the whole list -- what a caller does with the compounds OnMouseDown /
    // OnMouseDownBodies / ExecuteFractureRoutine return.  The compounds come back in the order given; a compound named twice or out of
    // range throws Error(SURTR_E_INVALID).  The current event is replaced (LastCounts() are this call's).  A piece whose faces cannot
    // be extracted is flagged: as everywhere, that throws unless AllowFlagged(true); then it comes back without triangles and
    // LastFlagged().fragments names it by its position in the call's piece order.
    // withHulls: InitCompoundResult::Hull of every piece as well (surtr_event_hulls on the fragments the call presents).
    // cookUnusable (with withHulls): InitCompoundResult::Cooked for the pieces HullUsable refuses at cookArgs.HullRelTolerance, cooked
    // at cookArgs.CookWeldDistance / CookPlaneTolerance; hulls and cooker run behind each other on the device and come back in one
    // download (surtr_event_hulls_cook).  Every other member is what the call without the flag returns.
    std::vector<std::vector<InitCompoundResult>> InitCompounds(const std::vector<int>& compounds, bool renderConvex, bool withHulls = false,
                                                               bool cookUnusable = false, const FractureArgs& cookArgs = FractureArgs());
    std::vector<InitCompoundResult> InitCompound(int compound, bool renderConvex, bool withHulls = false);
    // ---- bodies that move (Update writes each body's pose into m_structuredBufferData[i].WorldMatrix, Src/Surtr.cpp:347-352) ----
    // One rigid pose per compound of the scene (surtr_scene_set_poses: Matrix::m in the layout TransformCompound takes); the resident
    // pieces stay in the frame they were committed in.  ApplyPose bakes a compound's pose into its pieces (:1846-1851) and makes the
    // pose the identity; with the identity it does nothing at all.
    void SetPoses(const std::vector<Matrix>& world);
    std::vector<Matrix> Poses();
    void ApplyPose(int compound);
    void ApplyPoses(const std::vector<int>& compounds);      // the same for several, the derived data rebuilt once (surtr_scene_apply_poses)
    // OnMouseDown's queries on the bodies where their poses put them (surtr_scene_raycast / surtr_scene_overlap).  OverlapBodies: one
    // value per COMPOUND, 0 no piece of it is touched, 1 touched, 2 touched but the body's mass <= minMass (density 10; < 0: no gate).
    surtr_scene_ray_hit RaycastScene(const Vector3& origin, const Vector3& dir, float maxDist = 1000.f);
    std::vector<uint8_t> OverlapBodies(const Vector3& centre, float radius, float minMass = 1e-4f);
    // One record per compound in its body frame, added up on the device (surtr_scene_mass): what setMass / setCMassLocalPose /
    // setMassSpaceInertiaTensor take for a body whose pose the solver holds.
    std::vector<surtr_mass> BodyMassProperties(int set, float density = 10.f);
    // ---- scene upkeep (surtr_scene_bounds / _remove / _append / _cull): what a frame loop does besides clicking ----
    // BodyBounds: the world-space box of every compound under its pose, taken on the device (set 0 = Mesh, 1 = Convex): a broad
    // phase's, a renderer's and a kill volume's input.
    std::vector<surtr_bounds> BodyBounds(int set = 1);
    // Contacts: the pairs of pieces of two bodies that overlap or are within `margin` of each other, with distance, witness points and
    // normal, taken on the device from the Convex solids and the poses (surtr_scene_contacts), ascending by (piece_a, piece_b).
    // totals (may be null): the candidate counts of the broad and mid phases.  With ImpactsFromContacts below it is the front of a
    // frame loop: Contacts -> ImpactsFromContacts -> OnImpacts.
    std::vector<surtr_contact> Contacts(float margin, surtr_contact_header* totals = nullptr);
    // RemoveBodies: erases the listed compounds (any order; one out of range or named twice, or all of them, throws
    // Error(SURTR_E_INVALID)); the others keep their order and their poses.  No solid leaves the device.
    void RemoveBodies(const std::vector<int>& compounds);
    // AddBodies: push_back of new compounds from host pieces, vetted as SetCompound vets them; poses: one per new compound, or empty
    // for the identity.  Returns the number of the first new compound.  A refused call leaves the scene as it was.
    int AddBodies(const std::vector<Compound>& compoundVec, const std::vector<Matrix>& poses = {});
    // CullBodies: removes the bodies of mass <= minMass (Convex set, density 10: the gate of Src/Surtr.cpp:228 as a removal rule;
    // minMass < 0: none) and, with keepBox = {lo, hi}, those whose Convex bounds are disjoint from it.  Returns the reason bits per
    // compound as numbered BEFORE the removal (SURTR_CULL_*).  When every body is marked nothing is removed and Error(SURTR_E_INVALID)
    // is thrown.  apply = false only marks.
    std::vector<uint8_t> CullBodies(float minMass = 1e-4f, const std::pair<Vector3, Vector3>* keepBox = nullptr, bool apply = true);
    // OnMouseDown's picking with the reference's semantics (:207-233): the ray is cast on the posed scene; a hit sets
    // args.ImpactPosition = hit + dir * args.TargetAdder; with args.RadialMode the compounds whose body mask is 1 for the sphere of
    // radius args.ImpactRadius / 2 are returned (the gate is on the mass of the BODY), else the compound hit.  Ascending.
    // hit / bodyMask (may be null) receive the ray's record and the sphere's body mask (asked for, it is taken without RadialMode too).
    std::vector<int> PickBodies(const Vector3& origin, const Vector3& dir, FractureArgs& args, surtr_scene_ray_hit* hit = nullptr,
                                std::vector<uint8_t>* bodyMask = nullptr);
    // PickBodies, then ExecuteFractureRoutine (which bakes the stored pose first) in descending compound number.  hit / bodyMask:
    // what the pick it acted on found.  oneEvent: as for OnMouseDown.
    std::vector<int> OnMouseDownBodies(const Vector3& origin, const Vector3& dir, FractureArgs& args, float maxAxisScale,
                                       const std::vector<Vector3>& spherePointCloud, std::vector<int>* hitCompounds = nullptr,
                                       surtr_scene_ray_hit* hit = nullptr, std::vector<uint8_t>* bodyMask = nullptr, bool oneEvent = false);
    // ---- several impacts in one frame (the contact callback behind setContactReportThreshold, Src/Surtr.cpp:1163, 2518) ----
    // ExecuteFractureRoutine for the impacts a solver reported in one frame, in ONE pass (surtr_scene_fracture_impacts): the pattern
    // and the modes come from `args`, position and radius from each impact; the pattern is placed per impact at maxAxisScale * 2
    // around its position and the cloud scaled and shifted per impact (:1911-1915).  The compounds of an impact may come in any order
    // (sorted descending); one named twice, inside one impact or under two, throws Error(SURTR_E_INVALID), as does an impact without
    // a compound.  In order: ApplyPoses over all of them, one placement launch, one mask launch when PartialFracture, one event, one
    // regrouping with each body's own sphere, one refit, one commit.  Returns the compounds made: the scene is the one the
    // several-compound routine called per impact, in the order given, leaves.  When the event flagged a unit and AllowFlagged is off,
    // NOTHING is committed.
    // When an impact sets `pattern` or `partial`, the frame takes the pattern library instead: one instance of each impact's own
    // stored pattern (surtr_place_cells_patterns), the mask bytes of the impacts that are not partial cleared, one event over every
    // cell of every instance, the regrouping with a flag per impact (surtr_event_regroup_impacts_partial).  An impact that leaves
    // `pattern` at -1 there uses the installed pattern, which is stored for it once.  The installed pattern stays installed.
    // LastCellBase(): the first global cell of every instance of the last such frame (n + 1 entries).
    std::vector<int> ExecuteFractureRoutine(const std::vector<Impact>& impacts, float maxAxisScale, const FractureArgs& args,
                                            const std::vector<Vector3>& spherePointCloud);
    // The contact callback's work: which bodies does each sphere reach (ONE surtr_scene_overlap call with all the spheres, each of
    // radius `radius / 2` as in PickBodies, with PickBodies' gate on the body's mass), then the routine above (oneEvent) or the
    // several-compound routine per impact in the order given.  Only position and radius of `spheres` are read.  A body reached by
    // several impacts goes to the FIRST of them in list order: the later ones do not see it (sequentially they would meet its
    // fragments; that takes a second call).  An impact left without a body is dropped.  acted (may be null) receives the impacts as
    // they ran.  Returns the compounds made, numbered as after the last commit.
    // Impacts that set `pattern` or `partial` keep them.  With oneEvent off such a frame runs the sequential cycles with SelectPattern
    // before each and the impact's own flag in its args; the pattern installed before the call is installed again after it.
    std::vector<int> OnImpacts(const std::vector<Impact>& spheres, const FractureArgs& args, float maxAxisScale,
                               const std::vector<Vector3>& spherePointCloud, std::vector<Impact>* acted = nullptr, bool oneEvent = true);
    const std::vector<uint32_t>& LastCellBase() const { return cell_base_; }
    surtr_counts LastCounts() const { return counts_; }
    // The degenerate policy at this level (include/surtr_hip.h, surtr_counts::n_failed): where the reference leaves its own
    // arrays the engine flags the unit instead of emulating what the reference's memory happens to hold -- a flagged (cell,
    // piece) pair yields NO fragment, a flagged fragment keeps its un-refitted Convex / has no triangles.  A caller must not
    // lose pieces without knowing: by default ApplyFracture / PrepareFracture / DoFracture THROW Error(SURTR_E_TOPOLOGY) when
    // the event flagged anything (the reference's own signal on that path is `throw std::exception()`, Src/Poly.cpp:258);
    // after AllowFlagged(true) they return what is valid and LastFlagged() names what was left out.
    struct FlaggedUnits { uint32_t n_failed = 0; std::vector<std::pair<int, int>> pairs /* (cell, piece): no fragment */; std::vector<uint32_t> fragments /* output index */; };
    void AllowFlagged(bool allow) { allow_flagged_ = allow; }
    const FlaggedUnits& LastFlagged() const { return flagged_; }
    // How many engines the host keeps busy on this GPU at once (surtr_set_events_in_flight: no result changes, events of a few
    // hundred pairs then take the kernels that leave the other engines room).  The reference runs one event at a time.
    // FractureArgs::RefittingPointLimit for RefitSolid, RefittingTask (on the default engine) and events with refit; DoFracture
    // sets it from its `args`.  4 .. 32, anything else throws Error(SURTR_E_INVALID).
    void SetRefittingPointLimit(int n) { check(surtr_set_refit_point_limit(ctx_, n < 0 ? 0u : (uint32_t)n), "surtr_set_refit_point_limit"); }
    int RefittingPointLimit() { uint32_t n = 4; check(surtr_get_refit_point_limit(ctx_, &n), "surtr_get_refit_point_limit"); return (int)n; }
    void SetEventsInFlight(uint32_t n) { check(surtr_set_events_in_flight(ctx_, n), "surtr_set_events_in_flight"); }
    surtr_ctx* Raw() { return ctx_; }

private:
    void check(int rc, const char* what);
    std::vector<Fragment> download_fragments(bool render);
    void report_flagged(const std::vector<Fragment>& frags, uint32_t cellBegin, uint32_t cellEnd, const char* what);
    // what the three ExecuteFractureRoutine share (surtr_host.cpp)
    static std::vector<float> placed_cloud(const std::vector<Vector3>& spherePointCloud, float radius, const Vector3& position);
    std::vector<int> regroup_refit_commit(const char* what, const std::function<int(uint32_t*, uint32_t*, uint32_t*, int32_t*, uint32_t*, uint32_t*)>& regroup);
    std::vector<int> fracture_descending(const std::vector<int>& hit, float maxAxisScale, const FractureArgs& args, const std::vector<Vector3>& spherePointCloud);
    std::vector<uint8_t> two_call_mask(const char* what, const std::function<int(uint32_t, uint32_t*, uint8_t*)>& call);
    std::vector<uint8_t> outside_mask(const std::vector<uint32_t>& t, const std::vector<float>& fc, const float org[3], float radius);
    bool allow_flagged_ = false;
    bool render_normals_ = false;
    FlaggedUnits flagged_;
    surtr_ctx* ctx_ = nullptr;
    void check_impact_patterns(const std::vector<Impact>& impacts);
    int installed_pattern_id();      // the library id of the installed pattern, stored now if it is not yet
    int installed_id_ = -1;          // ... -1: not stored, or another pattern has been installed since
    int pair_partial_ = -1, pair_general_ = -1;      // UsePatternPair
    std::vector<uint32_t> cell_base_;
    uint32_t n_cells_ = 0, n_pieces_ = 0;
    surtr_counts counts_{};
};

} // namespace surtr
