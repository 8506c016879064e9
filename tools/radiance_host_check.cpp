// Stand-alone check of rtiRadianceHost and its argument checks (include/srt_radiance.h), meant for a
// sanitizer build of the library's host code (make asan): the Cornell box at 48 x 32 under a spot and
// a point light, a hemisphere of S = 7 with rotations and the mirror, with and without modulate and an
// in-place blend, every refusal once, and the call against its own composition
// (rtaRaysHost -> rtrClosestHost -> rthLightHitsHost -> the ordered sum) on every bit.
//   make asan
//   hipcc -Xarch_host -fsanitize=address,undefined -Iinclude tools/radiance_host_check.cpp \
//       -Lsimpleraytracer_amd/lib_asan -lModelRunner -Wl,-rpath,$PWD/simpleraytracer_amd/lib_asan -o radiance_host_check
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "srt_query.h"
#include "srt_radiance.h"
#include "srt_rays.h"

namespace {

int failures = 0;

void Expect(bool ok, const char* what) {
    if (!ok) {
        std::printf("FAILED: %s (%s)\n", what, srtGetLastError());
        ++failures;
    }
}

void Refused(int rc, const char* text) {
    const bool ok = rc == -1 && std::strstr(srtGetLastError(), text) != nullptr;
    if (!ok) {
        std::printf("FAILED: expected a refusal naming \"%s\", got rc %d and \"%s\"\n", text, rc, srtGetLastError());
        ++failures;
    }
}

}  // namespace

int main(int argc, char** argv) {
    const std::string path = std::string(argc > 1 ? argv[1] : ".") + "/radiance_host_check_cornell.srt";
    Expect(srtWriteScene(path.c_str(), SRT_SCENE_CORNELL, 0, 0, 0.f) == 0, "srtWriteScene");
    const size_t W = 48, H = 32, count = W * H;
    std::vector<float> pos(count * 2);
    for (size_t y = 0; y < H; ++y) {
        for (size_t x = 0; x < W; ++x) {
            pos[2 * (y * W + x)] = (static_cast<float>(x) + 0.5f) / static_cast<float>(W);
            pos[2 * (y * W + x) + 1] = (static_cast<float>(y) + 0.5f) / static_cast<float>(H);
        }
    }
    std::vector<int> ids(count);
    std::vector<float> depth(count);
    Expect(rtqQueryHost(path.c_str(), W, H, pos.data(), count, ids.data(), depth.data()) == 0, "rtqQueryHost");
    ids[0] = -1, ids[1] = 12, ids[2] = 0x7FFFFFFF;  // (no surface: nothing is read through these)

    rtd_light_host lights[2] = {};
    lights[0].struct_size = sizeof(rtd_light_host);
    lights[0].kind = 0;
    const float cam[10] = {0.4f, 1.2f, 0.6f, 0.0f, 0.6f, 2.7f, 0.0f, 1.0f, 0.0f, 70.0f};
    std::memcpy(lights[0].camera10, cam, sizeof cam);
    lights[0].width = 64, lights[0].height = 48;
    lights[0].color[0] = 1.0f, lights[0].color[1] = 0.9f, lights[0].color[2] = 0.8f;
    lights[0].bias = 1.0f / 128.0f;
    lights[1].struct_size = sizeof(rtd_light_host);
    lights[1].kind = 1;
    lights[1].origin[0] = 0.0f, lights[1].origin[1] = 1.0f, lights[1].origin[2] = 2.7f;
    lights[1].face_size = 32;
    lights[1].color[0] = 0.3f, lights[1].color[1] = 0.5f, lights[1].color[2] = 0.9f;
    lights[1].falloff = 2.0f, lights[1].bias = 1.0f / 128.0f;
    const float ambient[3] = {0.05f, 0.04f, 0.03f};

    const unsigned S = 7;
    std::vector<float> samples(S * 3), rotations(RTA_ROTATIONS * 2);
    for (unsigned s = 0; s < S; ++s) {  // (directions in the upper hemisphere; they need not be unit for this check)
        const float a = 0.9f * static_cast<float>(s), r = 0.2f + 0.1f * static_cast<float>(s);
        samples[3 * s] = r * std::cos(a), samples[3 * s + 1] = r * std::sin(a);
        samples[3 * s + 2] = std::sqrt(1.0f - r * r);
    }
    for (unsigned k = 0; k < RTA_ROTATIONS; ++k) {
        rotations[2 * k] = std::cos(0.4f * static_cast<float>(k)), rotations[2 * k + 1] = std::sin(0.4f * static_cast<float>(k));
    }
    rta_generator gen = {};
    gen.struct_size = sizeof gen;
    gen.kind = RTA_HEMISPHERE;
    gen.samples = S;
    gen.d_samples = samples.data();
    gen.d_rotations = rotations.data();
    gen.tmin = 1.0f / 1024.0f, gen.tmax = 4.0f;

    std::vector<float> rgba(count * 4), want(count * 4);
    Expect(rtiRadianceHost(path.c_str(), W, H, lights, 2, ambient, pos.data(), ids.data(), count, &gen, nullptr, rgba.data()) == 0,
           "rtiRadianceHost");
    // the composition
    std::vector<float> rays(static_cast<size_t>(S) * count * 8), t(S * count), lit(S * count * 4);
    std::vector<int> hit(S * count);
    Expect(rtaRaysHost(path.c_str(), W, H, pos.data(), ids.data(), count, &gen, rays.data()) == 0, "rtaRaysHost");
    Expect(rtrClosestHost(path.c_str(), rays.data(), S * count, hit.data(), t.data(), nullptr) == 0, "rtrClosestHost");
    Expect(rthLightHitsHost(path.c_str(), lights, 2, ambient, rays.data(), hit.data(), t.data(), S * count, nullptr, lit.data(),
                            nullptr) == 0,
           "rthLightHitsHost");
    size_t on_surface = 0, partial = 0;
    for (size_t q = 0; q < count; ++q) {
        bool on = false;
        for (int k = 0; k < 8; ++k) {
            on = on || rays[8 * q + k] != 0.f;
        }
        float sum[3] = {0.f, 0.f, 0.f};
        unsigned hits = 0;
        for (unsigned s = 0; s < S; ++s) {
            const float* c = lit.data() + 4 * (s * count + q);
            for (int k = 0; k < 3; ++k) {
                sum[k] = sum[k] + c[k];
            }
            hits += c[3] >= 0.f ? 1u : 0u;
        }
        for (int k = 0; k < 3; ++k) {
            want[4 * q + k] = on ? sum[k] / static_cast<float>(S) : 0.f;
        }
        want[4 * q + 3] = on ? static_cast<float>(hits) / static_cast<float>(S) : 0.f;
        on_surface += on ? 1 : 0;
        partial += on && hits > 0 && hits < S ? 1 : 0;
    }
    Expect(std::memcmp(rgba.data(), want.data(), rgba.size() * sizeof(float)) == 0, "the call equals its composition on every bit");
    Expect(on_surface >= 32 && partial >= 32, "the case has surfaces and partly hit elements");

    // modulate, and a blend in place against the blend out of place
    rth_blend blend = {sizeof(rth_blend), nullptr, {0.5f, 0.25f, 2.0f}};
    std::vector<float> base(count * 4), apart(count * 4);
    for (size_t i = 0; i < base.size(); ++i) {
        base[i] = 0.001f * static_cast<float>(i % 997);
    }
    blend.d_base = base.data();
    rti_options options = {sizeof(rti_options), 1, &blend};
    Expect(rtiRadianceHost(path.c_str(), W, H, lights, 2, ambient, pos.data(), ids.data(), count, &gen, &options, apart.data()) == 0,
           "modulate and blend");
    std::vector<float> within = base;
    blend.d_base = within.data();
    Expect(rtiRadianceHost(path.c_str(), W, H, lights, 2, ambient, pos.data(), ids.data(), count, &gen, &options, within.data()) == 0,
           "blend in place");
    Expect(std::memcmp(within.data(), apart.data(), apart.size() * sizeof(float)) == 0, "in place equals out of place");
    Expect(std::memcmp(apart.data(), base.data(), 3 * 4 * sizeof(float)) == 0, "elements off a surface keep the base element");
    blend.d_base = base.data();

    // the mirror, zero lights, zero elements
    rta_generator mirror = gen;
    mirror.kind = RTA_MIRROR, mirror.samples = 1, mirror.d_samples = nullptr, mirror.d_rotations = nullptr;
    Expect(rtiRadianceHost(path.c_str(), W, H, nullptr, 0, ambient, pos.data(), ids.data(), count, &mirror, nullptr, rgba.data()) == 0,
           "the mirror without lights");
    Expect(rtiRadianceHost(path.c_str(), W, H, lights, 2, ambient, nullptr, nullptr, 0, &gen, nullptr, nullptr) == 0, "no elements");

    // refusals
    auto call = [&](const rta_generator* g, const rti_options* o) {
        return rtiRadianceHost(path.c_str(), W, H, lights, 2, ambient, pos.data(), ids.data(), count, g, o, rgba.data());
    };
    rta_generator bad = gen;
    bad.kind = RTA_AREA;
    Refused(call(&bad, nullptr), "rta_generator.kind is RTA_AREA");
    bad = gen, bad.samples = 0;
    Refused(call(&bad, nullptr), "rta_generator.samples must be 1 to 64, got 0");
    bad = gen, bad.samples = 65;
    Refused(call(&bad, nullptr), "rta_generator.samples must be 1 to 64, got 65");
    bad = mirror, bad.samples = 2;
    Refused(call(&bad, nullptr), "rta_generator.samples must be 1 for RTA_MIRROR, got 2");
    Refused(call(nullptr, nullptr), "gen is NULL");
    rti_options wrong = options;
    wrong.struct_size = 8;
    Refused(call(&gen, &wrong), "rti_options.struct_size is 8");
    rth_blend small = blend;
    small.struct_size = 8;
    wrong = options, wrong.blend = &small;
    Refused(call(&gen, &wrong), "rth_blend.struct_size is 8");
    small = blend, small.weight[1] = NAN;
    Refused(call(&gen, &wrong), "weight value 1 is not finite");
    small = blend, small.d_base = nullptr;
    Refused(call(&gen, &wrong), "blend->d_base is NULL");
    Refused(rtiRadianceHost(nullptr, W, H, lights, 2, ambient, pos.data(), ids.data(), count, &gen, nullptr, rgba.data()),
            "scene_path is NULL");
    Refused(rtiRadianceHost(path.c_str(), W, H, lights, 2, ambient, pos.data(), ids.data(), count, &gen, nullptr, nullptr),
            "rgba is NULL");
    Refused(rtiRadianceFrameAsync(nullptr, nullptr, 0, ambient, nullptr, nullptr, 0, 0, &gen, nullptr, nullptr, nullptr),
            "Bad scene handle");
    std::remove(path.c_str());
    std::printf("radiance_host_check: %d failure(s); %zu of %zu elements on a surface, %zu partly hit\n", failures, on_surface, count,
                partial);
    return failures == 0 ? 0 : 1;
}
