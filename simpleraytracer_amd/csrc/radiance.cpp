// Sampled radiance on the host (radiance.h HostRadiance; include/srt_radiance.h rtiRadianceHost): the
// composition the answer is defined as, made of the host answers of the three families it joins,
// then the ordered sum. DESIGN.md section 2 "Radiance".
#include "radiance.h"

#include <vector>

#include "hits_math.h"
#include "visibility_math.h"

namespace srt {

void HostRadiance(const Scene& scene, std::size_t width, std::size_t height, const HostLight* lights, std::size_t count,
                  const float ambient[3], const float* positions, const int* ids, std::size_t elements,
                  const VisibilityGen& gen, const RadianceStore& store) {
    if (elements == 0) {
        return;
    }
    const std::size_t S = gen.count, rays_count = S * elements;
    // Steps 1 to 3: the rays, their closest hits, the hits under the lights (unblended).
    std::vector<float> rays(rays_count * 8), t(rays_count), lit(rays_count * 4);
    std::vector<int> hit(rays_count);
    HostVisibilityRays(scene, width, height, positions, ids, elements, gen, rays.data());
    HostRayClosest(scene, rays.data(), rays_count, hit.data(), t.data(), nullptr, true);
    const float none[3] = {0.f, 0.f, 0.f};
    HostLightHits(scene, lights, count, ambient, rays.data(), hit.data(), t.data(), rays_count, nullptr, none, lit.data(),
                  nullptr);
    const Frame f = MakeFrame(scene.camera, width, height);
    const std::size_t n = scene.triangle_count();
    for (std::size_t q = 0; q < elements; ++q) {
        const int id = ids[q];
        bool on = false;  // on a surface in the visibility family's sense: nothing is read through id otherwise
        if (id >= 0 && static_cast<std::size_t>(id) < n) {
            on = VisibilitySurfaceAt(f.origin, f.base, f.du, f.dv, scene.vertices.data() + 9 * static_cast<std::size_t>(id),
                                     positions[2 * q], positions[2 * q + 1])
                     .valid;
        }
        float out[4] = {0.f, 0.f, 0.f, 0.f};
        if (on) {
            // Steps 4 and 5: ascending s, one addition per sample and channel.
            float sum[3] = {0.f, 0.f, 0.f};
            unsigned hits = 0;
            for (std::size_t s = 0; s < S; ++s) {
                const float* c = lit.data() + 4 * (s * elements + q);
                for (int k = 0; k < 3; ++k) {
                    sum[k] = sum[k] + c[k];
                }
                hits += c[3] >= 0.f ? 1u : 0u;
            }
            const float* al = scene.albedo.data() + 3 * static_cast<std::size_t>(id);
            for (int k = 0; k < 3; ++k) {
                const float m = sum[k] / static_cast<float>(S);
                out[k] = store.modulate ? al[k] * m : m;
            }
            out[3] = static_cast<float>(hits) / static_cast<float>(S);
        }
        if (store.base != nullptr) {
            const float* b = store.base + 4 * q;
            const float base[4] = {b[0], b[1], b[2], b[3]};
            HitBlend(!on, base, store.weight, out);
        }
        for (int k = 0; k < 4; ++k) {
            store.rgba[4 * q + k] = out[k];
        }
    }
}

}  // namespace srt
