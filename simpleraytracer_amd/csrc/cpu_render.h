// Host (CPU) backend of an ml_model: BASELINE config C1 ("test_app single-triangle 256x256 CPU
// render, runs without a GPU"). Selected explicitly -- ML_VISIBLE_DEVICES=cpu (or set and empty,
// SURVEY.md section 8(b)) -- never as a silent fallback: without a HIP device and without that
// selection mlSetModelInputInfo fails with the HIP error.
//
// Same canonical arithmetic as the HIP kernels (bit for bit): edge records
// with explicit fma, the exact test E_A, E_B, E_C >= 0, det > 0, t = vol / det, lexicographic
// (t, id) minimum, headlight shading. A software rasterizer around it: each record's screen box
// (the kernels' double-precision solve) bins it to 16 x 16 pixel tiles whose ray boxes it can
// overlap, and each tile's pixels test only their tile's records (tiles whose rays leave the
// screen-box range test every record). Threads over tiles. Not the oracle (oracle/srt_oracle.c,
// test infrastructure, plain brute force); the tests compare the two.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "scene.h"

namespace srt {

// A record's screen box on the host (the kernels' ComputeRecord choice): mode 0 = the float fast
// path (screen_box.h) where it applies, else the double solve; 1 = the double solve; 2 = the fast
// path only (false where it does not apply). box = (xlo, xhi, ylo, yhi).
bool HostScreenBox(const float c[9], int mode, float box[4]);

// The closest hit at `count` image positions (fx, fy) of the scene's width x height frame, brute
// force over every record with the canonical math (the host answer of a point query: render.h
// LaunchQuery): ids[i] = the hit triangle or -1, t[i] = its t or +inf.
void HostClosestHits(const Scene& scene, std::size_t width, std::size_t height, const float* positions,
                     std::size_t count, int* ids, float* t);

// The surface attributes (gbuffer_math.h) of `count` (position, triangle id) pairs of the scene's
// width x height frame (the host answer of the G-buffer: render.h LaunchGBuffer), into the planes
// that are non-null: depth[count], bary[count][2], normal[count][4], albedo[count][4]. An id outside
// the scene gives the miss values.
void HostGBuffer(const Scene& scene, std::size_t width, std::size_t height, const float* positions, const int* ids,
                 std::size_t count, float* depth, float* bary, float* normal, float* albedo);

// The vertex attributes (surface_math.h) of `count` (position, triangle id) pairs of the scene's
// width x height frame (the host answer of render.h LaunchSurface): the caller's corner normals
// (n x 9), corner uvs (n x 6) and texture (tex_height x tex_width x 4), each null for none, under
// `flags` (surface_math.h kSurface*), into the planes that are non-null: normal[count][4],
// albedo[count][4], rgba[count][4], uv[count][2]. An id outside the scene gives the miss values.
void HostSurface(const Scene& scene, std::size_t width, std::size_t height, const float* positions, const int* ids,
                 std::size_t count, const float* normals, const float* uvs, const float* texture,
                 std::size_t tex_width, std::size_t tex_height, unsigned flags, float* normal, float* albedo,
                 float* rgba, float* uv);

// The interpolation of one corner table (n x 3 x channels) at the pairs (the host answer of render.h
// LaunchInterpolate): out[count][channels]; an id outside the scene gives zeros.
void HostInterpolate(const Scene& scene, std::size_t width, std::size_t height, const float* positions, const int* ids,
                     std::size_t count, const float* table, std::size_t channels, float* out);

// The resolve of `samples` sample planes of the band rows [row_begin, row_begin + row_count) of the
// scene's width x height frame (the host answer of render.h LaunchResolve; samples_math.h):
// offsets[s] (row_count x width x 2) and ids[s] (row_count x width), band-local, into rgba
// (row_count x width x 4) -- the mean of the shaded samples, alpha = the share that hit. An id
// outside the scene is a miss.
void HostResolve(const Scene& scene, std::size_t width, std::size_t height, const float* const* offsets,
                 const int* const* ids, std::size_t samples, std::size_t row_begin, std::size_t row_count, float* rgba);

// The `layers` nearest hits, front to back, at `count` image positions of the scene's width x
// height frame, brute force over every record with the canonical math (the host answer of render.h
// LaunchLayers): ids[k * count + i] = layer k's triangle or -1, t[...] (null: not stored) = its t or
// +inf -- the k-th smallest (t, id) among the triangles passing the exact test.
void HostLayers(const Scene& scene, std::size_t width, std::size_t height, const float* positions, std::size_t count,
                std::size_t layers, int* ids, float* t);

// The over-composite (layers_math.h; the host answer of render.h LaunchComposite) of `layers` id
// planes (ids: layers x row_count x width) of the band rows [row_begin, row_begin + row_count) of
// the scene's width x height frame under the opacity table (one float per triangle): offsets
// (row_count x width x 2), band-local, into rgba (row_count x width x 4).
void HostComposite(const Scene& scene, std::size_t width, std::size_t height, const float* offsets, const int* ids,
                   std::size_t layers, const float* opacity, std::size_t row_begin, std::size_t row_count,
                   float* rgba);

// The spot-light shadow mask (shadow_math.h; the host answer of render.h LaunchShadow) of the band
// rows [row_begin, row_begin + row_count) of the scene's width x height frame, the light being the
// same triangles' light_width x light_height frame under light_camera: offsets (row_count x width x
// 2) and ids (row_count x width), band-local, into mask (row_count x width classes) and -- non-null --
// rgba (row_count x width x 4). The light frame's closest hit by brute force over every record.
void HostShadow(const Scene& scene, std::size_t width, std::size_t height, const Camera& light_camera,
                std::size_t light_width, std::size_t light_height, const float* offsets, const int* ids,
                std::size_t row_begin, std::size_t row_count, float bias, unsigned char* mask, float* rgba, float dim);
// The omni-light shadow mask (omni_math.h; the host answer of render.h LaunchOmniShadow): HostShadow
// under the point light at `origin`, six cube faces of face_size x face_size; `face` (may be null)
// receives the face each pixel selected, 255 for a class-3 pixel.
void HostOmniShadow(const Scene& scene, std::size_t width, std::size_t height, const float origin[3],
                    std::size_t face_size, const float* offsets, const int* ids, std::size_t row_begin,
                    std::size_t row_count, float bias, unsigned char* mask, unsigned char* face, float* rgba, float dim);
// Face `face` (0 .. 5) of the light at `origin` as a camera (omni_math.h OmniFaceCamera).
Camera OmniFaceCameraOf(const float origin[3], int face);

// Direct lighting (lighting_math.h; the host answer of render.h LaunchLighting): the lit RGBA of the
// band under `count` lights of the same triangles, a spot light being `camera` at width x height, a
// point light `origin` with six face_size x face_size cube faces. offsets, ids: HostShadow's; rgba
// (row_count x width x 4); classes (count x row_count x width, light-major) may be null. Every light
// frame's closest hit by brute force over every record.
struct HostLight {
    bool point;
    Camera camera;              // spot
    std::size_t width, height;  // spot
    float origin[3];            // point
    std::size_t face_size;      // point
    float color[3];
    float falloff, bias;
};
void HostLighting(const Scene& scene, std::size_t width, std::size_t height, const HostLight* lights, std::size_t count,
                  const float ambient[3], const float* offsets, const int* ids, std::size_t row_begin,
                  std::size_t row_count, float* rgba, unsigned char* classes);

// Lit surfaces (material_math.h; the host answer of render.h LaunchLitSurface): HostLighting with the
// pixel's normal and albedo taken from HostSurface's tables (`surface`; null: none, the shading
// table's) and, with a `material`, a Blinn-Phong term. Without both it is HostLighting, bit for bit.
struct HostSurfaceTables {  // HostSurface's inputs: host arrays, each null for none
    const float* normals;
    const float* uvs;
    const float* texture;
    std::size_t tex_width, tex_height;
    unsigned flags;
};
struct HostMaterial {
    float specular[3];
    int shininess_log2;  // 0 .. kMaterialMaxShininessLog2
};
void HostLitSurface(const Scene& scene, std::size_t width, std::size_t height, const HostLight* lights, std::size_t count,
                    const float ambient[3], const HostSurfaceTables* surface, const HostMaterial* material,
                    const float* offsets, const int* ids, std::size_t row_begin, std::size_t row_count, float* rgba,
                    unsigned char* classes);

// Lit ray hits (hits_math.h; the host answer of render.h LaunchLightHits): HostLighting for `elements`
// hits given as (ray, id, t) -- rays elements x 8, ids and t elements each -- with the surface point
// from the element's own ray; no view frame. base (elements x 4; null: store; may be rgba) with
// weight[3]: the element is added onto it. classes (count x elements, light-major) may be null.
void HostLightHits(const Scene& scene, const HostLight* lights, std::size_t count, const float ambient[3],
                   const float* rays, const int* ids, const float* t, std::size_t elements, const float* base,
                   const float weight[3], float* rgba, unsigned char* classes);

// The light frame's projection rows (px, py, pz) as HostShadow and LaunchShadow compute them.
void HostShadowRows(const Camera& light_camera, std::size_t light_width, std::size_t light_height, float rows[9]);

// Whether env ML_VISIBLE_DEVICES selects the CPU backend ("cpu", or set to the empty string).
bool CpuBackendSelected();

class CpuRenderer {
public:
    explicit CpuRenderer(const Scene& scene);
    void Configure(std::size_t width, std::size_t height);
    bool configured() const { return m_width != 0; }
    // host offsets (H x W x 2) -> host RGBA (H x W x 4); element types from the scene's flags
    // (float, or IEEE binary16 bit patterns).
    void Render(const void* host_offsets, void* host_rgba);
    static unsigned Threads();  // env SRT_CPU_THREADS, else OMP_NUM_THREADS, else the host's cores

private:
    const Scene& m_scene;
    bool m_in_half = false;
    bool m_out_half = false;
    std::size_t m_width = 0;
    std::size_t m_height = 0;
};

}  // namespace srt
