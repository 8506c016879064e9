#include "cpu_render.h"

#include "gbuffer_math.h"
#include "hits_math.h"
#include "layers_math.h"
#include "lighting_math.h"
#include "material_math.h"
#include "omni_math.h"
#include "samples_math.h"
#include "screen_box.h"
#include "shading_normal.h"
#include "shadow_math.h"
#include "surface_math.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <thread>

namespace srt {
namespace {

constexpr int kTile = 16;             // pixels per tile side
constexpr float kScreenRange = 4.0f;  // render.h kScreenBoxRange: screen boxes bound |fx|, |fy| <= 4

// The kernels' expressions (render.hip Dot3 / Cross3 / ComputeRecord / ScreenBox / ShadePixel),
// restated for the host: explicit fma, no contraction (-ffp-contract=off), IEEE divide and sqrt.
inline float Dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return std::fma(az, bz, std::fma(ay, by, ax * bx));
}
inline void Cross3(float ax, float ay, float az, float bx, float by, float bz, float& cx, float& cy, float& cz) {
    cx = ay * bz - az * by;
    cy = az * bx - ax * bz;
    cz = ax * by - ay * bx;
}

// Double -> float rounded toward -inf / +inf (the device's __double2float_rd / _ru).
inline float DownF(double v) {
    float f = static_cast<float>(v);
    if (static_cast<double>(f) > v) {
        f = std::nextafter(f, -std::numeric_limits<float>::infinity());
    }
    return f;
}
inline float UpF(double v) {
    float f = static_cast<float>(v);
    if (static_cast<double>(f) < v) {
        f = std::nextafter(f, std::numeric_limits<float>::infinity());
    }
    return f;
}

struct Box {
    float xlo, xhi, ylo, yhi;
};

// Every (fx, fy) with |fx|, |fy| <= 4 at which the float edge tests of c can all pass lies in
// this box (render.hip ScreenBox: the pairwise line intersections of the slack-shifted edges,
// solved in double, padded, rounded outward); unbounded when it cannot be bounded.
Box ScreenBox(const float c[9]) {
    const float inf = std::numeric_limits<float>::infinity();
    const Box unbounded{-inf, inf, -inf, inf};
    double gx[3], gy[3], k[3];
    for (int e = 0; e < 3; ++e) {
        const double c0 = c[3 * e], cx = c[3 * e + 1], cy = c[3 * e + 2];
        if (!(std::fabs(c0) < 1e30 && std::fabs(cx) < 1e30 && std::fabs(cy) < 1e30)) {
            return unbounded;
        }
        gx[e] = cx;
        gy[e] = cy;
        const double slack = (0x1p-24 * (std::fabs(c0) + kScreenRange * std::fabs(cx)) + 0x1p-120) * (1.0 + 1e-12);
        k[e] = c0 + slack;
    }
    const double dAB = gx[0] * gy[1] - gy[0] * gx[1];
    const double dBC = gx[1] * gy[2] - gy[1] * gx[2];
    const double dCA = gx[2] * gy[0] - gy[2] * gx[0];
    const bool spans = (dAB > 0 && dBC > 0 && dCA > 0) || (dAB < 0 && dBC < 0 && dCA < 0);
    if (!spans) {
        return unbounded;
    }
    double xlo = 1e300, xhi = -1e300, ylo = 1e300, yhi = -1e300;
    const double dv[3] = {dBC, dCA, dAB};
    for (int v = 0; v < 3; ++v) {
        const int i = (v + 1) % 3, j = (v + 2) % 3;
        const double inv = 1.0 / dv[v], ainv = std::fabs(inv);
        if (!(ainv < 1e300)) {
            return unbounded;
        }
        const double tx1 = -k[i] * gy[j], tx2 = k[j] * gy[i];
        const double ty1 = -gx[i] * k[j], ty2 = gx[j] * k[i];
        const double x = (tx1 + tx2) * inv, y = (ty1 + ty2) * inv;
        const double px = 1e-12 * ((std::fabs(tx1) + std::fabs(tx2)) * ainv + std::fabs(x)) + 1e-300;
        const double py = 1e-12 * ((std::fabs(ty1) + std::fabs(ty2)) * ainv + std::fabs(y)) + 1e-300;
        xlo = std::fmin(xlo, x - px);
        xhi = std::fmax(xhi, x + px);
        ylo = std::fmin(ylo, y - py);
        yhi = std::fmax(yhi, y + py);
    }
    if (!(xlo <= xhi && ylo <= yhi)) {
        return unbounded;
    }
    return Box{DownF(xlo), UpF(xhi), DownF(ylo), UpF(yhi)};
}

// One triangle's record: edge coefficients c, vol, screen box, shading normal (n, |n|).
struct Rec {
    float c[9];
    float vol;
    Box sb;
    float n[4];
};

Rec MakeRecord(const float* v, const Frame& f) {
    Rec r;
    const float qnan = std::numeric_limits<float>::quiet_NaN();
    const float inf = std::numeric_limits<float>::infinity();
    const float ax = v[0] - f.origin[0], ay = v[1] - f.origin[1], az = v[2] - f.origin[2];
    const float bx = v[3] - f.origin[0], by = v[4] - f.origin[1], bz = v[5] - f.origin[2];
    const float cx = v[6] - f.origin[0], cy = v[7] - f.origin[1], cz = v[8] - f.origin[2];
    float n[9];
    Cross3(bx, by, bz, cx, cy, cz, n[0], n[1], n[2]);
    Cross3(cx, cy, cz, ax, ay, az, n[3], n[4], n[5]);
    Cross3(ax, ay, az, bx, by, bz, n[6], n[7], n[8]);
    float vol = Dot3(ax, ay, az, n[0], n[1], n[2]);
    const bool disabled = !(std::isfinite(vol) && vol != 0.f);
    if (disabled) {
        std::fill(r.c, r.c + 9, qnan);
        r.vol = qnan;
        r.sb = Box{inf, -inf, inf, -inf};
    } else {
        if (vol < 0.f) {
            for (float& x : n) {
                x = -x;
            }
            vol = -vol;
        }
        for (int e = 0; e < 3; ++e) {
            const float nx = n[3 * e], ny = n[3 * e + 1], nz = n[3 * e + 2];
            r.c[3 * e + 0] = Dot3(nx, ny, nz, f.base[0], f.base[1], f.base[2]);
            r.c[3 * e + 1] = Dot3(nx, ny, nz, f.du[0], f.du[1], f.du[2]);
            r.c[3 * e + 2] = Dot3(nx, ny, nz, f.dv[0], f.dv[1], f.dv[2]);
        }
        r.vol = vol;
        float fb[4];
        r.sb = ScreenBoxFast(r.c, kScreenRange, fb) ? Box{fb[0], fb[1], fb[2], fb[3]} : ScreenBox(r.c);
    }
    const float e1x = v[3] - v[0], e1y = v[4] - v[1], e1z = v[5] - v[2];
    const float e2x = v[6] - v[0], e2y = v[7] - v[1], e2z = v[8] - v[2];
    Cross3(e1x, e1y, e1z, e2x, e2y, e2z, r.n[0], r.n[1], r.n[2]);
    r.n[3] = std::sqrt(Dot3(r.n[0], r.n[1], r.n[2], r.n[0], r.n[1], r.n[2]));
    return r;
}

// Runs f(i) for i in [0, n) over the backend's threads (work handed out in chunks).
template <class F>
void ParallelFor(std::size_t n, std::size_t chunk, F&& f) {
    const unsigned threads = std::max(1u, std::min<unsigned>(CpuRenderer::Threads(),
                                                             static_cast<unsigned>((n + chunk - 1) / chunk)));
    std::atomic<std::size_t> next{0};
    auto work = [&] {
        for (;;) {
            const std::size_t b = next.fetch_add(chunk);
            if (b >= n) {
                return;
            }
            for (std::size_t i = b; i < std::min(n, b + chunk); ++i) {
                f(i);
            }
        }
    };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < threads; ++t) {
        pool.emplace_back(work);
    }
    work();
    for (auto& t : pool) {
        t.join();
    }
}

}  // namespace

bool HostScreenBox(const float c[9], int mode, float box[4]) {
    if (mode != 1 && ScreenBoxFast(c, kScreenRange, box)) {
        return true;
    }
    if (mode == 2) {
        return false;
    }
    const Box b = ScreenBox(c);
    box[0] = b.xlo;
    box[1] = b.xhi;
    box[2] = b.ylo;
    box[3] = b.yhi;
    return true;
}

void HostClosestHits(const Scene& scene, std::size_t width, std::size_t height, const float* positions,
                     std::size_t count, int* ids, float* t) {
    if (width == 0 || height == 0) {
        throw std::runtime_error("Host query: frame dimensions must be non-zero");
    }
    const Frame f = MakeFrame(scene.camera, width, height);
    const std::size_t n = scene.triangle_count();
    std::vector<Rec> recs(n);
    ParallelFor(n, 1024, [&](std::size_t i) { recs[i] = MakeRecord(scene.vertices.data() + 9 * i, f); });
    ParallelFor(count, 64, [&](std::size_t q) {
        const float px = positions[2 * q], py = positions[2 * q + 1];
        float best = std::numeric_limits<float>::infinity();
        int id = -1;
        for (std::size_t k = 0; k < n; ++k) {  // ascending ids: strict < keeps the lowest on ties
            const float* c = recs[k].c;
            const float eA = std::fma(py, c[2], std::fma(px, c[1], c[0]));
            const float eB = std::fma(py, c[5], std::fma(px, c[4], c[3]));
            const float eC = std::fma(py, c[8], std::fma(px, c[7], c[6]));
            if (eA >= 0.f && eB >= 0.f && eC >= 0.f) {
                const float det = (eA + eB) + eC;
                if (det > 0.f) {
                    const float tt = recs[k].vol / det;
                    if (tt < best) {
                        best = tt;
                        id = static_cast<int>(k);
                    }
                }
            }
        }
        ids[q] = id;
        t[q] = best;
    });
}

void HostGBuffer(const Scene& scene, std::size_t width, std::size_t height, const float* positions, const int* ids,
                 std::size_t count, float* depth, float* bary, float* normal, float* albedo) {
    if (width == 0 || height == 0) {
        throw std::runtime_error("Host G-buffer: frame dimensions must be non-zero");
    }
    if (depth == nullptr && bary == nullptr && normal == nullptr && albedo == nullptr) {
        return;  // (no plane: nothing is read either)
    }
    const Frame f = MakeFrame(scene.camera, width, height);
    const std::size_t n = scene.triangle_count();
    ParallelFor(count, 256, [&](std::size_t q) {
        const int id = ids[q];
        GBufferTexel o = GBufferMiss(scene.background);
        if (id >= 0 && static_cast<std::size_t>(id) < n) {
            const Rec r = MakeRecord(scene.vertices.data() + 9 * static_cast<std::size_t>(id), f);
            const float* a = scene.albedo.data() + 3 * static_cast<std::size_t>(id);
            o = GBufferHit(r.c, r.vol, f.base, f.du, f.dv, positions[2 * q], positions[2 * q + 1], id, r.n[0], r.n[1],
                           r.n[2], r.n[3], a[0], a[1], a[2]);
        }
        if (depth != nullptr) {
            depth[q] = o.depth;
        }
        if (bary != nullptr) {
            bary[2 * q] = o.w1;
            bary[2 * q + 1] = o.w2;
        }
        if (normal != nullptr) {
            const float v[4] = {o.nx, o.ny, o.nz, o.cosv};
            std::copy(v, v + 4, normal + 4 * q);
        }
        if (albedo != nullptr) {
            const float v[4] = {o.r, o.g, o.b, o.a};
            std::copy(v, v + 4, albedo + 4 * q);
        }
    });
}

namespace {

void CheckSurfaceTables(const HostSurfaceTables& s) {
    if ((s.flags & ~kSurfaceFlags) != 0u) {
        throw std::runtime_error("Host surface: unknown flags");
    }
    if (s.texture != nullptr && (s.uvs == nullptr || s.tex_width < 1 || s.tex_width > kSurfaceMaxTexture ||
                                 s.tex_height < 1 || s.tex_height > kSurfaceMaxTexture)) {
        throw std::runtime_error("Host surface: a texture needs uvs and 1 to 16384 texels per side");
    }
}

// What the surface of triangle i looks like at (fx, fy), r being its record under frame f: the normal
// plane on[4], the albedo plane's colour oa[3] and the uv (surface_math.h; HostSurface, HostLitSurface).
void SurfaceLook(const Scene& scene, const Frame& f, const HostSurfaceTables& s, std::size_t i, const Rec& r, float fx,
                 float fy, float on[4], float oa[3], float ouv[2]) {
    const bool clamp = (s.flags & kSurfaceWrapClamp) != 0u, nearest = (s.flags & kSurfaceFilterNearest) != 0u;
    const bool modulate = (s.flags & kSurfaceModulate) != 0u;
    const int tw = static_cast<int>(s.tex_width), th = static_cast<int>(s.tex_height);
    const SurfaceWeights bw = SurfaceBary(r.c, fx, fy);
    const float* a = scene.albedo.data() + 3 * i;
    if (s.normals != nullptr) {
        const float* cn = s.normals + 9 * i;
        const SurfaceNormal sn = SurfaceSmoothNormal(SurfaceMix(bw, cn[0], cn[3], cn[6]), SurfaceMix(bw, cn[1], cn[4], cn[7]),
                                                     SurfaceMix(bw, cn[2], cn[5], cn[8]), f.base, f.du, f.dv, fx, fy);
        const float v[4] = {sn.x, sn.y, sn.z, sn.cosv};
        std::copy(v, v + 4, on);
    } else {
        const GBufferTexel g = GBufferHit(r.c, r.vol, f.base, f.du, f.dv, fx, fy, static_cast<int>(i), r.n[0], r.n[1],
                                          r.n[2], r.n[3], a[0], a[1], a[2]);
        const float v[4] = {g.nx, g.ny, g.nz, g.cosv};
        std::copy(v, v + 4, on);
    }
    ouv[0] = ouv[1] = 0.f;
    if (s.uvs != nullptr) {
        const float* ct = s.uvs + 6 * i;
        ouv[0] = SurfaceMix(bw, ct[0], ct[2], ct[4]);
        ouv[1] = SurfaceMix(bw, ct[1], ct[3], ct[5]);
    }
    std::copy(a, a + 3, oa);
    if (s.texture != nullptr) {
        float tex[3];
        if (nearest) {
            const int ti = SurfaceNearest(SurfaceWrap(ouv[0], clamp), tw);
            const int tj = SurfaceNearest(SurfaceWrap(ouv[1], clamp), th);
            const float* t = s.texture + 4 * (static_cast<std::size_t>(tj) * s.tex_width + static_cast<std::size_t>(ti));
            std::copy(t, t + 3, tex);
        } else {
            const SurfaceTaps sx = SurfaceBilinear(SurfaceWrap(ouv[0], clamp), tw, clamp);
            const SurfaceTaps sy = SurfaceBilinear(SurfaceWrap(ouv[1], clamp), th, clamp);
            const float* top = s.texture + 4 * static_cast<std::size_t>(sy.i0) * s.tex_width;
            const float* bot = s.texture + 4 * static_cast<std::size_t>(sy.i1) * s.tex_width;
            for (int c = 0; c < 3; ++c) {
                tex[c] = SurfaceLerp(SurfaceLerp(top[4 * sx.i0 + c], top[4 * sx.i1 + c], sx.a),
                                     SurfaceLerp(bot[4 * sx.i0 + c], bot[4 * sx.i1 + c], sx.a), sy.a);
            }
        }
        for (int c = 0; c < 3; ++c) {
            oa[c] = modulate ? tex[c] * a[c] : tex[c];
        }
    }
}

}  // namespace

void HostSurface(const Scene& scene, std::size_t width, std::size_t height, const float* positions, const int* ids,
                 std::size_t count, const float* normals, const float* uvs, const float* texture,
                 std::size_t tex_width, std::size_t tex_height, unsigned flags, float* normal, float* albedo,
                 float* rgba, float* uv) {
    if (width == 0 || height == 0) {
        throw std::runtime_error("Host surface: frame dimensions must be non-zero");
    }
    const HostSurfaceTables tables{normals, uvs, texture, tex_width, tex_height, flags};
    CheckSurfaceTables(tables);
    if (normal == nullptr && albedo == nullptr && rgba == nullptr && uv == nullptr) {
        return;  // (no plane: nothing is read either)
    }
    const Frame f = MakeFrame(scene.camera, width, height);
    const std::size_t n = scene.triangle_count();
    ParallelFor(count, 256, [&](std::size_t q) {
        const int id = ids[q];
        float on[4] = {0.f, 0.f, 0.f, 1.f};
        float oa[4] = {scene.background[0], scene.background[1], scene.background[2], -1.f};
        float ouv[2] = {0.f, 0.f};
        if (id >= 0 && static_cast<std::size_t>(id) < n) {
            const std::size_t i = static_cast<std::size_t>(id);
            const Rec r = MakeRecord(scene.vertices.data() + 9 * i, f);
            SurfaceLook(scene, f, tables, i, r, positions[2 * q], positions[2 * q + 1], on, oa, ouv);
            oa[3] = static_cast<float>(id);
        }
        if (normal != nullptr) {
            std::copy(on, on + 4, normal + 4 * q);
        }
        if (albedo != nullptr) {
            std::copy(oa, oa + 4, albedo + 4 * q);
        }
        if (rgba != nullptr) {
            const float v[4] = {oa[0] * on[3], oa[1] * on[3], oa[2] * on[3], oa[3]};
            std::copy(v, v + 4, rgba + 4 * q);
        }
        if (uv != nullptr) {
            uv[2 * q] = ouv[0];
            uv[2 * q + 1] = ouv[1];
        }
    });
}

void HostInterpolate(const Scene& scene, std::size_t width, std::size_t height, const float* positions, const int* ids,
                     std::size_t count, const float* table, std::size_t channels, float* out) {
    if (width == 0 || height == 0) {
        throw std::runtime_error("Host interpolation: frame dimensions must be non-zero");
    }
    if (channels < 1 || channels > static_cast<std::size_t>(kSurfaceMaxChannels)) {
        throw std::runtime_error("Host interpolation: channels must be 1 to 4");
    }
    const Frame f = MakeFrame(scene.camera, width, height);
    const std::size_t n = scene.triangle_count();
    ParallelFor(count, 256, [&](std::size_t q) {
        const int id = ids[q];
        float* o = out + channels * q;
        std::fill(o, o + channels, 0.f);
        if (id >= 0 && static_cast<std::size_t>(id) < n) {
            const std::size_t i = static_cast<std::size_t>(id);
            const Rec r = MakeRecord(scene.vertices.data() + 9 * i, f);
            const SurfaceWeights bw = SurfaceBary(r.c, positions[2 * q], positions[2 * q + 1]);
            const float* a = table + 3 * channels * i;
            for (std::size_t c = 0; c < channels; ++c) {
                o[c] = SurfaceMix(bw, a[c], a[channels + c], a[2 * channels + c]);
            }
        }
    });
}

void HostResolve(const Scene& scene, std::size_t width, std::size_t height, const float* const* offsets,
                 const int* const* ids, std::size_t samples, std::size_t row_begin, std::size_t row_count, float* rgba) {
    if (width == 0 || height == 0) {
        throw std::runtime_error("Host resolve: frame dimensions must be non-zero");
    }
    if (samples == 0) {
        throw std::runtime_error("Host resolve: samples must be positive");
    }
    if (row_begin > height || row_count > height - row_begin) {
        throw std::runtime_error("Host resolve: row band outside the frame");
    }
    const Frame f = MakeFrame(scene.camera, width, height);
    const std::size_t n = scene.triangle_count();
    const float wf = static_cast<float>(width), hf = static_cast<float>(height);
    const ResolveRgb miss{scene.background[0], scene.background[1], scene.background[2]};
    ParallelFor(row_count * width, 1024, [&](std::size_t i) {
        const unsigned x = static_cast<unsigned>(i % width), y = static_cast<unsigned>(row_begin + i / width);
        ResolveAcc acc{};
        for (std::size_t s = 0; s < samples; ++s) {
            const int id = ids[s][i];
            const bool hit = id >= 0 && static_cast<std::size_t>(id) < n;
            ResolveRgb c = miss;
            if (hit) {
                const Rec r = MakeRecord(scene.vertices.data() + 9 * static_cast<std::size_t>(id), f);
                const float* a = scene.albedo.data() + 3 * static_cast<std::size_t>(id);
                float fx, fy;
                ResolvePosition(x, y, offsets[s][2 * i], offsets[s][2 * i + 1], wf, hf, fx, fy);
                c = ResolveShadeHit(f.base, f.du, f.dv, fx, fy, r.n[0], r.n[1], r.n[2], r.n[3], a[0], a[1], a[2]);
            }
            ResolveAdd(acc, static_cast<unsigned>(s), c, hit);
        }
        const ResolveTexel t = ResolveFinish(acc, static_cast<unsigned>(samples));
        const float v[4] = {t.r, t.g, t.b, t.a};
        std::copy(v, v + 4, rgba + 4 * i);
    });
}

void HostLayers(const Scene& scene, std::size_t width, std::size_t height, const float* positions, std::size_t count,
                std::size_t layers, int* ids, float* t) {
    if (width == 0 || height == 0) {
        throw std::runtime_error("Host layers: frame dimensions must be non-zero");
    }
    if (layers == 0) {
        throw std::runtime_error("Host layers: layers must be positive");
    }
    const Frame f = MakeFrame(scene.camera, width, height);
    const std::size_t n = scene.triangle_count();
    std::vector<Rec> recs(n);
    ParallelFor(n, 1024, [&](std::size_t i) { recs[i] = MakeRecord(scene.vertices.data() + 9 * i, f); });
    const float inf = std::numeric_limits<float>::infinity();
    ParallelFor(count, 64, [&](std::size_t q) {
        const float px = positions[2 * q], py = positions[2 * q + 1];
        // The `layers` smallest (t, id) so far, ascending; ids ascend, so a later record goes behind
        // every held one of equal t (strict <).
        std::vector<float> bt(layers, inf);
        std::vector<int> bi(layers, -1);
        for (std::size_t k = 0; k < n; ++k) {
            const float* c = recs[k].c;
            const float eA = std::fma(py, c[2], std::fma(px, c[1], c[0]));
            const float eB = std::fma(py, c[5], std::fma(px, c[4], c[3]));
            const float eC = std::fma(py, c[8], std::fma(px, c[7], c[6]));
            if (eA >= 0.f && eB >= 0.f && eC >= 0.f) {
                const float det = (eA + eB) + eC;
                if (det > 0.f) {
                    const float tt = recs[k].vol / det;
                    if (tt < bt[layers - 1]) {
                        std::size_t j = layers - 1;
                        for (; j > 0 && tt < bt[j - 1]; --j) {
                            bt[j] = bt[j - 1];
                            bi[j] = bi[j - 1];
                        }
                        bt[j] = tt;
                        bi[j] = static_cast<int>(k);
                    }
                }
            }
        }
        for (std::size_t k = 0; k < layers; ++k) {
            ids[k * count + q] = bi[k];
            if (t != nullptr) {
                t[k * count + q] = bt[k];
            }
        }
    });
}

void HostComposite(const Scene& scene, std::size_t width, std::size_t height, const float* offsets, const int* ids,
                   std::size_t layers, const float* opacity, std::size_t row_begin, std::size_t row_count,
                   float* rgba) {
    if (width == 0 || height == 0) {
        throw std::runtime_error("Host composite: frame dimensions must be non-zero");
    }
    if (layers == 0) {
        throw std::runtime_error("Host composite: layers must be positive");
    }
    if (row_begin > height || row_count > height - row_begin) {
        throw std::runtime_error("Host composite: row band outside the frame");
    }
    const Frame f = MakeFrame(scene.camera, width, height);
    const std::size_t n = scene.triangle_count();
    const float wf = static_cast<float>(width), hf = static_cast<float>(height);
    const std::size_t plane = row_count * width;
    ParallelFor(plane, 1024, [&](std::size_t i) {
        const unsigned x = static_cast<unsigned>(i % width), y = static_cast<unsigned>(row_begin + i / width);
        float fx, fy;
        ResolvePosition(x, y, offsets[2 * i], offsets[2 * i + 1], wf, hf, fx, fy);
        CompositeAcc acc = CompositeStart();
        for (std::size_t k = 0; k < layers; ++k) {
            const int id = ids[k * plane + i];
            if (id < 0 || static_cast<std::size_t>(id) >= n) {
                break;
            }
            const Rec r = MakeRecord(scene.vertices.data() + 9 * static_cast<std::size_t>(id), f);
            const float* a = scene.albedo.data() + 3 * static_cast<std::size_t>(id);
            const ResolveRgb c = ResolveShadeHit(f.base, f.du, f.dv, fx, fy, r.n[0], r.n[1], r.n[2], r.n[3], a[0], a[1], a[2]);
            CompositeAdd(acc, opacity[id], c);
        }
        const ResolveTexel o = CompositeFinish(acc, scene.background);
        const float v[4] = {o.r, o.g, o.b, o.a};
        std::copy(v, v + 4, rgba + 4 * i);
    });
}

void HostShadowRows(const Camera& light_camera, std::size_t light_width, std::size_t light_height, float rows[9]) {
    if (light_width == 0 || light_height == 0) {
        throw std::runtime_error("Host shadow: light frame dimensions must be non-zero");
    }
    const Frame lf = MakeFrame(light_camera, light_width, light_height);
    ShadowProjectionRows(lf.base, lf.du, lf.dv, rows);
}

void HostShadow(const Scene& scene, std::size_t width, std::size_t height, const Camera& light_camera,
                std::size_t light_width, std::size_t light_height, const float* offsets, const int* ids,
                std::size_t row_begin, std::size_t row_count, float bias, unsigned char* mask, float* rgba, float dim) {
    if (width == 0 || height == 0 || light_width == 0 || light_height == 0) {
        throw std::runtime_error("Host shadow: frame dimensions must be non-zero");
    }
    if (row_begin > height || row_count > height - row_begin) {
        throw std::runtime_error("Host shadow: row band outside the frame");
    }
    const Frame f = MakeFrame(scene.camera, width, height);
    const Frame lf = MakeFrame(light_camera, light_width, light_height);
    float rows[9];
    ShadowProjectionRows(lf.base, lf.du, lf.dv, rows);
    const std::size_t n = scene.triangle_count();
    std::vector<Rec> lrecs(n);  // every triangle's record under the light frame
    ParallelFor(n, 1024, [&](std::size_t i) { lrecs[i] = MakeRecord(scene.vertices.data() + 9 * i, lf); });
    const float wf = static_cast<float>(width), hf = static_cast<float>(height);
    const float inf = std::numeric_limits<float>::infinity();
    ParallelFor(row_count * width, 64, [&](std::size_t i) {
        const std::size_t x = i % width, y = row_begin + i / width;
        const int id = ids[i];
        const float fx = (static_cast<float>(x) + offsets[2 * i]) / wf;
        const float fy = (static_cast<float>(y) + offsets[2 * i + 1]) / hf;
        const bool surface = id >= 0 && static_cast<std::size_t>(id) < n;
        unsigned char cls = kShadowNoSurface;
        float out[4] = {scene.background[0], scene.background[1], scene.background[2], -1.f};
        if (surface) {
            const Rec r = MakeRecord(scene.vertices.data() + 9 * static_cast<std::size_t>(id), f);
            const float t = ShadowDepth(r.c, r.vol, fx, fy);
            const ShadowPoint sp = ShadowProject(f.origin, f.base, f.du, f.dv, fx, fy, t, lf.origin, rows, bias);
            cls = kShadowOutside;
            if (sp.inside) {
                float best = inf;
                int lid = -1;
                for (std::size_t k = 0; k < n; ++k) {  // ascending ids: strict < keeps the lowest on ties
                    const float* c = lrecs[k].c;
                    const float eA = std::fma(sp.gy, c[2], std::fma(sp.gx, c[1], c[0]));
                    const float eB = std::fma(sp.gy, c[5], std::fma(sp.gx, c[4], c[3]));
                    const float eC = std::fma(sp.gy, c[8], std::fma(sp.gx, c[7], c[6]));
                    if (eA >= 0.f && eB >= 0.f && eC >= 0.f) {
                        const float det = (eA + eB) + eC;
                        if (det > 0.f) {
                            const float tt = lrecs[k].vol / det;
                            if (tt < best) {
                                best = tt;
                                lid = static_cast<int>(k);
                            }
                        }
                    }
                }
                cls = ShadowClass(id, lid, best, sp.thr);
            }
            if (rgba != nullptr) {
                const float* a = scene.albedo.data() + 3 * static_cast<std::size_t>(id);
                const ResolveRgb c = ResolveShadeHit(f.base, f.du, f.dv, fx, fy, r.n[0], r.n[1], r.n[2], r.n[3], a[0], a[1], a[2]);
                const float k = ShadowScale(cls, dim);
                out[0] = c.r * k;
                out[1] = c.g * k;
                out[2] = c.b * k;
                out[3] = static_cast<float>(id);
            }
        }
        mask[i] = cls;
        if (rgba != nullptr) {
            std::copy(out, out + 4, rgba + 4 * i);
        }
    });
}

Camera OmniFaceCameraOf(const float origin[3], int face) {
    float c10[10];
    OmniFaceCamera(origin, face, c10);
    Camera c{};
    std::copy(c10, c10 + 3, c.eye);
    std::copy(c10 + 3, c10 + 6, c.lookat);
    std::copy(c10 + 6, c10 + 9, c.up);
    c.vfov_deg = c10[9];
    return c;
}

void HostOmniShadow(const Scene& scene, std::size_t width, std::size_t height, const float origin[3],
                    std::size_t face_size, const float* offsets, const int* ids, std::size_t row_begin,
                    std::size_t row_count, float bias, unsigned char* mask, unsigned char* face, float* rgba, float dim) {
    if (width == 0 || height == 0 || face_size == 0) {
        throw std::runtime_error("Host omni shadow: frame dimensions must be non-zero");
    }
    if (row_begin > height || row_count > height - row_begin) {
        throw std::runtime_error("Host omni shadow: row band outside the frame");
    }
    const Frame f = MakeFrame(scene.camera, width, height);
    const std::size_t n = scene.triangle_count();
    Frame lf[kOmniFaces];
    float rows[kOmniFaces][9];
    std::vector<Rec> lrecs(kOmniFaces * n);  // every triangle's record under every face frame
    for (int k = 0; k < kOmniFaces; ++k) {
        lf[k] = MakeFrame(OmniFaceCameraOf(origin, k), face_size, face_size);
        ShadowProjectionRows(lf[k].base, lf[k].du, lf[k].dv, rows[k]);
        Rec* out = lrecs.data() + static_cast<std::size_t>(k) * n;
        ParallelFor(n, 1024, [&](std::size_t i) { out[i] = MakeRecord(scene.vertices.data() + 9 * i, lf[k]); });
    }
    const float wf = static_cast<float>(width), hf = static_cast<float>(height);
    const float inf = std::numeric_limits<float>::infinity();
    ParallelFor(row_count * width, 64, [&](std::size_t i) {
        const std::size_t x = i % width, y = row_begin + i / width;
        const int id = ids[i];
        const float fx = (static_cast<float>(x) + offsets[2 * i]) / wf;
        const float fy = (static_cast<float>(y) + offsets[2 * i + 1]) / hf;
        const bool surface = id >= 0 && static_cast<std::size_t>(id) < n;
        unsigned char cls = kShadowNoSurface;
        unsigned char fc = kOmniNoFace;
        float out[4] = {scene.background[0], scene.background[1], scene.background[2], -1.f};
        if (surface) {
            const Rec r = MakeRecord(scene.vertices.data() + 9 * static_cast<std::size_t>(id), f);
            const float t = ShadowDepth(r.c, r.vol, fx, fy);
            float q[3];
            ShadowOffset(f.origin, f.base, f.du, f.dv, fx, fy, t, lf[0].origin, q);
            fc = static_cast<unsigned char>(OmniFace(q));
            const ShadowPoint sp = ShadowProjectOffset(q, rows[fc], bias);
            cls = kShadowOutside;
            if (sp.inside) {
                const Rec* recs = lrecs.data() + static_cast<std::size_t>(fc) * n;
                float best = inf;
                int lid = -1;
                for (std::size_t k = 0; k < n; ++k) {  // ascending ids: strict < keeps the lowest on ties
                    const float* c = recs[k].c;
                    const float eA = std::fma(sp.gy, c[2], std::fma(sp.gx, c[1], c[0]));
                    const float eB = std::fma(sp.gy, c[5], std::fma(sp.gx, c[4], c[3]));
                    const float eC = std::fma(sp.gy, c[8], std::fma(sp.gx, c[7], c[6]));
                    if (eA >= 0.f && eB >= 0.f && eC >= 0.f) {
                        const float det = (eA + eB) + eC;
                        if (det > 0.f) {
                            const float tt = recs[k].vol / det;
                            if (tt < best) {
                                best = tt;
                                lid = static_cast<int>(k);
                            }
                        }
                    }
                }
                cls = ShadowClass(id, lid, best, sp.thr);
            }
            if (rgba != nullptr) {
                const float* a = scene.albedo.data() + 3 * static_cast<std::size_t>(id);
                const ResolveRgb c = ResolveShadeHit(f.base, f.du, f.dv, fx, fy, r.n[0], r.n[1], r.n[2], r.n[3], a[0], a[1], a[2]);
                const float k = ShadowScale(cls, dim);
                out[0] = c.r * k;
                out[1] = c.g * k;
                out[2] = c.b * k;
                out[3] = static_cast<float>(id);
            }
        }
        mask[i] = cls;
        if (face != nullptr) {
            face[i] = fc;
        }
        if (rgba != nullptr) {
            std::copy(out, out + 4, rgba + 4 * i);
        }
    });
}

namespace {

// Every light's frames (1 or 6), their projection rows and every triangle's record under each.
struct HostLightFrame {
    Frame frame;
    float rows[9];
    std::vector<Rec> recs;
};
struct HostLightFrames {
    std::vector<HostLightFrame> frames;
    std::vector<std::size_t> first;  // per light
};
HostLightFrames MakeLightFrames(const Scene& scene, const HostLight* lights, std::size_t count) {
    const std::size_t n = scene.triangle_count();
    HostLightFrames all;
    all.first.resize(count);
    for (std::size_t l = 0; l < count; ++l) {
        const HostLight& in = lights[l];
        all.first[l] = all.frames.size();
        const int faces = in.point ? kOmniFaces : 1;
        for (int k = 0; k < faces; ++k) {
            HostLightFrame lf;
            lf.frame = in.point ? MakeFrame(OmniFaceCameraOf(in.origin, k), in.face_size, in.face_size)
                                : MakeFrame(in.camera, in.width, in.height);
            ShadowProjectionRows(lf.frame.base, lf.frame.du, lf.frame.dv, lf.rows);
            lf.recs.resize(n);
            Rec* out = lf.recs.data();
            const Frame& fr = lf.frame;
            ParallelFor(n, 1024, [&](std::size_t i) { out[i] = MakeRecord(scene.vertices.data() + 9 * i, fr); });
            all.frames.push_back(std::move(lf));
        }
    }
    return all;
}

// Light l at the surface point p of triangle id, whose geometric normal is nrm with nn = nrm.nrm and
// nd = nrm.d (lighting_math.h; the one statement of the rule for HostLitSurface and HostLightHits):
// q = p - origin, the light's class of p -- ShadowProjectOffset in its frame (the face OmniFace(q)
// of a point light), the frame's closest hit by brute force in ascending id, ShadowClass -- and,
// where the light contributes (class 1 and facing), its flat weight LightingWeight.
struct HostLightAt {
    unsigned char cls;
    bool contributes;
    float q[3], qq, w;  // qq, w: of a contributing light
};
HostLightAt LightAtPoint(const HostLightFrames& all, const HostLight& in, std::size_t l, std::size_t n, int id,
                         const float p[3], const float nrm[3], float nn, float nd) {
    const float inf = std::numeric_limits<float>::infinity();
    HostLightAt at{};
    const float* origin = all.frames[all.first[l]].frame.origin;
    for (int k = 0; k < 3; ++k) {
        at.q[k] = p[k] - origin[k];
    }
    const HostLightFrame& lf = all.frames[all.first[l] + (in.point ? static_cast<std::size_t>(OmniFace(at.q)) : 0)];
    const ShadowPoint sp = ShadowProjectOffset(at.q, lf.rows, in.bias);
    at.cls = kShadowOutside;
    if (sp.inside) {
        float best = inf;
        int lid = -1;
        for (std::size_t k = 0; k < n; ++k) {  // ascending ids: strict < keeps the lowest on ties
            const float* c = lf.recs[k].c;
            const float eA = std::fma(sp.gy, c[2], std::fma(sp.gx, c[1], c[0]));
            const float eB = std::fma(sp.gy, c[5], std::fma(sp.gx, c[4], c[3]));
            const float eC = std::fma(sp.gy, c[8], std::fma(sp.gx, c[7], c[6]));
            if (eA >= 0.f && eB >= 0.f && eC >= 0.f) {
                const float det = (eA + eB) + eC;
                if (det > 0.f) {
                    const float tt = lf.recs[k].vol / det;
                    if (tt < best) {
                        best = tt;
                        lid = static_cast<int>(k);
                    }
                }
            }
        }
        at.cls = ShadowClass(id, lid, best, sp.thr);
    }
    const float nl = ShadowDot(nrm, at.q);
    at.contributes = at.cls == kShadowLit && LightingFacing(nl, nd);
    if (at.contributes) {
        at.qq = ShadowDot(at.q, at.q);
        at.w = LightingWeight(nl, nn, at.qq, in.falloff);
    }
    return at;
}

}  // namespace

void HostLitSurface(const Scene& scene, std::size_t width, std::size_t height, const HostLight* lights, std::size_t count,
                    const float ambient[3], const HostSurfaceTables* surface, const HostMaterial* material,
                    const float* offsets, const int* ids, std::size_t row_begin, std::size_t row_count, float* rgba,
                    unsigned char* classes) {
    if (surface != nullptr) {
        CheckSurfaceTables(*surface);
    }
    if (material != nullptr && (material->shininess_log2 < 0 || material->shininess_log2 > kMaterialMaxShininessLog2)) {
        throw std::runtime_error("Host lighting: shininess_log2 outside 0 .. 12");
    }
    const HostSurfaceTables tables = surface != nullptr ? *surface : HostSurfaceTables{};
    const bool smooth = tables.normals != nullptr;
    if (width == 0 || height == 0) {
        throw std::runtime_error("Host lighting: frame dimensions must be non-zero");
    }
    if (row_begin > height || row_count > height - row_begin) {
        throw std::runtime_error("Host lighting: row band outside the frame");
    }
    const Frame f = MakeFrame(scene.camera, width, height);
    const std::size_t n = scene.triangle_count();
    const HostLightFrames frames = MakeLightFrames(scene, lights, count);
    const float wf = static_cast<float>(width), hf = static_cast<float>(height);
    const std::size_t plane = row_count * width;
    ParallelFor(plane, 64, [&](std::size_t i) {
        const std::size_t x = i % width, y = row_begin + i / width;
        const int id = ids[i];
        const float fx = (static_cast<float>(x) + offsets[2 * i]) / wf;
        const float fy = (static_cast<float>(y) + offsets[2 * i + 1]) / hf;
        const bool surface = id >= 0 && static_cast<std::size_t>(id) < n;
        float out[4] = {scene.background[0], scene.background[1], scene.background[2], -1.f};
        if (!surface) {
            for (std::size_t l = 0; l < count && classes != nullptr; ++l) {
                classes[l * plane + i] = kShadowNoSurface;
            }
            std::copy(out, out + 4, rgba + 4 * i);
            return;
        }
        const Rec r = MakeRecord(scene.vertices.data() + 9 * static_cast<std::size_t>(id), f);
        const float t = ShadowDepth(r.c, r.vol, fx, fy);
        float d[3], p[3];
        LightingPoint(f.origin, f.base, f.du, f.dv, fx, fy, t, d, p);
        const float nn = ShadowDot(r.n, r.n), nd = ShadowDot(r.n, d);
        float on[4], oa[3], ouv[2];
        SurfaceLook(scene, f, tables, static_cast<std::size_t>(id), r, fx, fy, on, oa, ouv);
        float e[3] = {ambient[0], ambient[1], ambient[2]}, sp[3] = {0.f, 0.f, 0.f};
        for (std::size_t l = 0; l < count; ++l) {
            const HostLight& in = lights[l];
            const HostLightAt at = LightAtPoint(frames, in, l, n, id, p, r.n, nn, nd);
            if (classes != nullptr) {
                classes[l * plane + i] = at.cls;
            }
            if (at.contributes) {
                const float w = smooth ? MaterialDiffuse(on, at.q, at.qq, in.falloff) : at.w;
                for (int k = 0; k < 3; ++k) {
                    e[k] = e[k] + in.color[k] * w;
                }
                if (material != nullptr && w > 0.f) {
                    const float ws = MaterialSpecular(on, at.q, at.qq, d, material->shininess_log2, in.falloff);
                    for (int k = 0; k < 3; ++k) {
                        sp[k] = sp[k] + in.color[k] * ws;
                    }
                }
            }
        }
        for (int k = 0; k < 3; ++k) {
            out[k] = material != nullptr ? oa[k] * e[k] + material->specular[k] * sp[k] : oa[k] * e[k];
        }
        out[3] = static_cast<float>(id);
        std::copy(out, out + 4, rgba + 4 * i);
    });
}

void HostLightHits(const Scene& scene, const HostLight* lights, std::size_t count, const float ambient[3],
                   const float* rays, const int* ids, const float* t, std::size_t elements, const float* base,
                   const float weight[3], float* rgba, unsigned char* classes) {
    const std::size_t n = scene.triangle_count();
    const HostLightFrames frames = MakeLightFrames(scene, lights, count);
    ParallelFor(elements, 64, [&](std::size_t i) {
        const float* o = rays + 8 * i;
        const float* d = o + 4;
        const int id = ids[i];
        const bool absent = HitAbsent(d);
        const bool surface = HitSurface(o, d, id, t[i], static_cast<unsigned>(n));
        float out[4] = {absent ? 0.f : scene.background[0], absent ? 0.f : scene.background[1],
                        absent ? 0.f : scene.background[2], -1.f};
        if (surface) {
            float p[3];
            HitPoint(o, d, t[i], p);
            const float4 nr = ShadingNormal(scene.vertices.data() + 9 * static_cast<std::size_t>(id));
            const float nrm[3] = {nr.x, nr.y, nr.z};
            const float* al = scene.albedo.data() + 3 * static_cast<std::size_t>(id);
            const float nn = ShadowDot(nrm, nrm), nd = ShadowDot(nrm, d);
            float e[3] = {ambient[0], ambient[1], ambient[2]};
            for (std::size_t l = 0; l < count; ++l) {
                const HostLightAt at = LightAtPoint(frames, lights[l], l, n, id, p, nrm, nn, nd);
                if (classes != nullptr) {
                    classes[l * elements + i] = at.cls;
                }
                if (at.contributes) {
                    for (int k = 0; k < 3; ++k) {
                        e[k] = e[k] + lights[l].color[k] * at.w;
                    }
                }
            }
            for (int k = 0; k < 3; ++k) {
                out[k] = al[k] * e[k];
            }
            out[3] = static_cast<float>(id);
        } else {
            for (std::size_t l = 0; l < count && classes != nullptr; ++l) {
                classes[l * elements + i] = kShadowNoSurface;
            }
        }
        if (base != nullptr) {
            const float b[4] = {base[4 * i], base[4 * i + 1], base[4 * i + 2], base[4 * i + 3]};
            HitBlend(absent, b, weight, out);
        }
        std::copy(out, out + 4, rgba + 4 * i);
    });
}

void HostLighting(const Scene& scene, std::size_t width, std::size_t height, const HostLight* lights, std::size_t count,
                  const float ambient[3], const float* offsets, const int* ids, std::size_t row_begin,
                  std::size_t row_count, float* rgba, unsigned char* classes) {
    HostLitSurface(scene, width, height, lights, count, ambient, nullptr, nullptr, offsets, ids, row_begin, row_count, rgba,
                   classes);
}

bool CpuBackendSelected() {
    const char* v = std::getenv("ML_VISIBLE_DEVICES");
    return v != nullptr && (*v == '\0' || std::strcmp(v, "cpu") == 0);
}

unsigned CpuRenderer::Threads() {
    for (const char* name : {"SRT_CPU_THREADS", "OMP_NUM_THREADS"}) {
        const char* v = std::getenv(name);
        if (v != nullptr && std::atoi(v) > 0) {
            return static_cast<unsigned>(std::atoi(v));
        }
    }
    const unsigned hw = std::thread::hardware_concurrency();
    return hw == 0 ? 1u : hw;
}

CpuRenderer::CpuRenderer(const Scene& scene)
    : m_scene(scene),
      m_in_half((scene.flags & kFlagInputFloat16) != 0u),
      m_out_half((scene.flags & kFlagOutputFloat16) != 0u) {}

void CpuRenderer::Configure(std::size_t width, std::size_t height) {
    if (width == 0 || height == 0) {
        throw std::runtime_error("CPU renderer: frame dimensions must be non-zero");
    }
    m_width = width;
    m_height = height;
}

void CpuRenderer::Render(const void* host_offsets, void* host_rgba) {
    if (!configured()) {
        throw std::runtime_error("Renderer used before Configure()");
    }
    const std::size_t W = m_width, H = m_height;
    const Frame f = MakeFrame(m_scene.camera, W, H);
    const float wf = static_cast<float>(W), hf = static_cast<float>(H);
    const std::size_t n = m_scene.triangle_count();
    // Records of every triangle (the kernels' record pass).
    std::vector<Rec> recs(n);
    ParallelFor(n, 1024, [&](std::size_t i) { recs[i] = MakeRecord(m_scene.vertices.data() + 9 * i, f); });
    // Ray positions (the kernels' GenerateRays) and each tile's ray box.
    std::vector<float> fx(W * H), fy(W * H);
    auto offset = [&](std::size_t i, int k) {
        if (m_in_half) {
            return static_cast<float>(static_cast<const _Float16*>(host_offsets)[2 * i + k]);
        }
        return static_cast<const float*>(host_offsets)[2 * i + k];
    };
    ParallelFor(H, 16, [&](std::size_t y) {
        for (std::size_t x = 0; x < W; ++x) {
            const std::size_t i = y * W + x;
            fx[i] = (static_cast<float>(x) + offset(i, 0)) / wf;
            fy[i] = (static_cast<float>(y) + offset(i, 1)) / hf;
        }
    });
    const std::size_t tx = (W + kTile - 1) / kTile, ty = (H + kTile - 1) / kTile, tiles = tx * ty;
    const float inf = std::numeric_limits<float>::infinity();
    std::vector<Box> tbox(tiles, Box{inf, -inf, inf, -inf});
    std::vector<char> usable(tiles, 0);
    ParallelFor(tiles, 8, [&](std::size_t t) {
        const std::size_t x0 = t % tx * kTile, y0 = t / tx * kTile;
        Box b{inf, -inf, inf, -inf};
        for (std::size_t y = y0; y < std::min(H, y0 + kTile); ++y) {
            for (std::size_t x = x0; x < std::min(W, x0 + kTile); ++x) {
                const float px = fx[y * W + x], py = fy[y * W + x];  // NaN drops out of fmin / fmax
                b = Box{std::fmin(b.xlo, px), std::fmax(b.xhi, px), std::fmin(b.ylo, py), std::fmax(b.yhi, py)};
            }
        }
        tbox[t] = b;
        usable[t] = b.xlo >= -kScreenRange && b.xhi <= kScreenRange && b.ylo >= -kScreenRange &&
                    b.yhi <= kScreenRange;
    });
    // Monotone column / row bounds of the usable tiles' boxes (suffix minimum of lo, prefix
    // maximum of hi): a record's candidate columns and rows by two binary searches each.
    std::vector<float> clo(tx, inf), chi(tx, -inf), rlo(ty, inf), rhi(ty, -inf);
    for (std::size_t t = 0; t < tiles; ++t) {
        if (usable[t] && tbox[t].xlo <= tbox[t].xhi) {
            const std::size_t c = t % tx, r = t / tx;
            clo[c] = std::min(clo[c], tbox[t].xlo);
            chi[c] = std::max(chi[c], tbox[t].xhi);
            rlo[r] = std::min(rlo[r], tbox[t].ylo);
            rhi[r] = std::max(rhi[r], tbox[t].yhi);
        }
    }
    for (std::size_t c = tx - 1; c-- > 0;) {
        clo[c] = std::min(clo[c], clo[c + 1]);
    }
    for (std::size_t c = 1; c < tx; ++c) {
        chi[c] = std::max(chi[c], chi[c - 1]);
    }
    for (std::size_t r = ty - 1; r-- > 0;) {
        rlo[r] = std::min(rlo[r], rlo[r + 1]);
    }
    for (std::size_t r = 1; r < ty; ++r) {
        rhi[r] = std::max(rhi[r], rhi[r - 1]);
    }
    // Bins: a record joins every usable tile whose box overlaps its screen box (ascending ids).
    // A pixel of a usable tile outside a record's screen box cannot pass its test (screen-box
    // guarantee), so skipping the pair is exact; tiles that are not usable test every record.
    std::vector<std::vector<std::uint32_t>> lists(tiles);
    for (std::size_t i = 0; i < n; ++i) {
        const Box& s = recs[i].sb;
        if (!(s.xlo <= s.xhi && s.ylo <= s.yhi)) {
            continue;  // disabled: never hits
        }
        const std::size_t c0 = std::lower_bound(chi.begin(), chi.end(), s.xlo) - chi.begin();
        const std::size_t c1 = std::upper_bound(clo.begin(), clo.end(), s.xhi) - clo.begin();
        const std::size_t r0 = std::lower_bound(rhi.begin(), rhi.end(), s.ylo) - rhi.begin();
        const std::size_t r1 = std::upper_bound(rlo.begin(), rlo.end(), s.yhi) - rlo.begin();
        for (std::size_t r = r0; r < r1; ++r) {
            for (std::size_t c = c0; c < c1; ++c) {
                const std::size_t t = r * tx + c;
                const Box& b = tbox[t];
                if (usable[t] && !(s.xhi < b.xlo || s.xlo > b.xhi || s.yhi < b.ylo || s.ylo > b.yhi)) {
                    lists[t].push_back(static_cast<std::uint32_t>(i));
                }
            }
        }
    }
    std::vector<std::uint32_t> all(n);
    for (std::size_t i = 0; i < n; ++i) {
        all[i] = static_cast<std::uint32_t>(i);
    }
    // Trace + shade, tile by tile.
    const float* albedo = m_scene.albedo.data();
    const float* bg = m_scene.background;
    ParallelFor(tiles, 1, [&](std::size_t t) {
        const std::vector<std::uint32_t>& cand = usable[t] ? lists[t] : all;
        const std::size_t x0 = t % tx * kTile, y0 = t / tx * kTile;
        for (std::size_t y = y0; y < std::min(H, y0 + kTile); ++y) {
            for (std::size_t x = x0; x < std::min(W, x0 + kTile); ++x) {
                const std::size_t p = y * W + x;
                const float px = fx[p], py = fy[p];
                float best = inf;
                int id = -1;
                for (const std::uint32_t k : cand) {  // ascending ids: strict < keeps the lowest on ties
                    const float* c = recs[k].c;
                    const float eA = std::fma(py, c[2], std::fma(px, c[1], c[0]));
                    const float eB = std::fma(py, c[5], std::fma(px, c[4], c[3]));
                    const float eC = std::fma(py, c[8], std::fma(px, c[7], c[6]));
                    if (eA >= 0.f && eB >= 0.f && eC >= 0.f) {
                        const float det = (eA + eB) + eC;
                        if (det > 0.f) {
                            const float tt = recs[k].vol / det;
                            if (tt < best) {
                                best = tt;
                                id = static_cast<int>(k);
                            }
                        }
                    }
                }
                float out[4];
                if (id < 0) {
                    out[0] = bg[0];
                    out[1] = bg[1];
                    out[2] = bg[2];
                    out[3] = -1.f;
                } else {
                    const float dx = std::fma(py, f.dv[0], std::fma(px, f.du[0], f.base[0]));
                    const float dy = std::fma(py, f.dv[1], std::fma(px, f.du[1], f.base[1]));
                    const float dz = std::fma(py, f.dv[2], std::fma(px, f.du[2], f.base[2]));
                    const float* nr = recs[id].n;
                    const float nd = Dot3(nr[0], nr[1], nr[2], dx, dy, dz);
                    const float dd = Dot3(dx, dy, dz, dx, dy, dz);
                    const float cosv = std::fmin(std::fabs(nd) / (nr[3] * std::sqrt(dd)), 1.f);
                    const float* a = albedo + 3 * static_cast<std::size_t>(id);
                    out[0] = a[0] * cosv;
                    out[1] = a[1] * cosv;
                    out[2] = a[2] * cosv;
                    out[3] = static_cast<float>(id);
                }
                if (m_out_half) {
                    _Float16* o = static_cast<_Float16*>(host_rgba) + 4 * p;
                    for (int k = 0; k < 4; ++k) {
                        o[k] = static_cast<_Float16>(out[k]);
                    }
                } else {
                    std::memcpy(static_cast<float*>(host_rgba) + 4 * p, out, sizeof(out));
                }
            }
        }
    });
}

}  // namespace srt
