// Extension C entry points (include/srt_render.h): scene files and device-level stages.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <exception>
#include <memory>
#include <string>
#include <vector>

#include "cpu_render.h"
#include "engine.h"
#include "lighting_math.h"
#include "material_math.h"
#include "omni_math.h"
#include "radiance.h"
#include "ray_math.h"
#include "rays.h"
#include "render.h"
#include "renderer.h"
#include "scene.h"
#include "srt_gbuffer.h"
#include "srt_hits.h"
#include "srt_layers.h"
#include "srt_light.h"
#include "srt_lighting.h"
#include "srt_material.h"
#include "srt_motion.h"
#include "srt_omni.h"
#include "srt_query.h"
#include "srt_pins.h"
#include "srt_radiance.h"
#include "srt_rays.h"
#include "srt_render.h"
#include "srt_samples.h"
#include "srt_surface.h"
#include "srt_visibility.h"
#include "surface_math.h"
#include "tile_lookup.h"
#include "visibility.h"
#include "visibility_math.h"

namespace {

thread_local std::string g_last_error;

template <class F>
int Guarded(F&& f) {
    try {
        f();
        g_last_error.clear();
        return 0;
    } catch (std::exception& e) {
        g_last_error = e.what();
    } catch (...) {
        g_last_error = "unknown error";
    }
    return -1;
}

srt::DeviceScene* FromHandle(srt_device_scene s) { return reinterpret_cast<srt::DeviceScene*>(s); }

// Binds the scene's device for the duration of a call, restoring the caller's device.
class Bind {
public:
    explicit Bind(int device) {
        if (hipGetDevice(&m_prev) != hipSuccess) {
            m_prev = -1;
        }
        srt::HipCheck(hipSetDevice(device), "hipSetDevice");
    }
    ~Bind() {
        if (m_prev >= 0) {
            (void)hipSetDevice(m_prev);
        }
    }

private:
    int m_prev = -1;
};

}  // namespace

extern "C" {

ML_API_ENTRY const char* srtGetLastError(void) { return g_last_error.c_str(); }

ML_API_ENTRY int srtWriteScene(const char* path, int kind, unsigned long long triangles, unsigned long long seed,
                               float size) {
    return Guarded([&] {
        if (path == nullptr) {
            throw std::runtime_error("Bad path argument");
        }
        srt::SaveScene(srt::MakeScene(kind, triangles, seed, size), path);
    });
}

ML_API_ENTRY int srtSceneTriangles(const char* path, unsigned long long* triangles) {
    return Guarded([&] {
        if (path == nullptr || triangles == nullptr) {
            throw std::runtime_error("Bad argument");
        }
        *triangles = srt::LoadScene(path).triangle_count();
    });
}

ML_API_ENTRY int srtReadScene(const char* path, unsigned long long capacity, unsigned long long* triangles,
                              float* vertices, float* albedo, float* camera10, float* background3,
                              unsigned* flags) {
    return Guarded([&] {
        if (path == nullptr) {
            throw std::runtime_error("Bad path argument");
        }
        const srt::Scene s = srt::LoadScene(path);
        const unsigned long long n = s.triangle_count();
        if (triangles != nullptr) {
            *triangles = n;
        }
        if ((vertices != nullptr || albedo != nullptr) && capacity < n) {
            throw std::runtime_error("Buffer too small: " + std::to_string(capacity) + " triangles for " +
                                     std::to_string(n));
        }
        if (vertices != nullptr) {
            std::copy(s.vertices.begin(), s.vertices.end(), vertices);
        }
        if (albedo != nullptr) {
            std::copy(s.albedo.begin(), s.albedo.end(), albedo);
        }
        if (camera10 != nullptr) {
            std::copy(s.camera.eye, s.camera.eye + 3, camera10);
            std::copy(s.camera.lookat, s.camera.lookat + 3, camera10 + 3);
            std::copy(s.camera.up, s.camera.up + 3, camera10 + 6);
            camera10[9] = s.camera.vfov_deg;
        }
        if (background3 != nullptr) {
            std::copy(s.background, s.background + 3, background3);
        }
        if (flags != nullptr) {
            *flags = s.flags;
        }
    });
}

ML_API_ENTRY int srtConvertScene(const char* src_path, const char* dst_path, int input_dtype, int output_dtype) {
    return Guarded([&] {
        if (src_path == nullptr || dst_path == nullptr) {
            throw std::runtime_error("Bad path argument");
        }
        srt::Scene s = srt::LoadScene(src_path);
        auto set = [&](int dtype, std::uint32_t bit, const char* what) {
            if (dtype == -1) {
                return;
            }
            if (dtype != ML_FLOAT32 && dtype != ML_FLOAT16) {
                throw std::runtime_error(std::string("Bad ") + what + " data type " + std::to_string(dtype));
            }
            s.flags = dtype == ML_FLOAT16 ? (s.flags | bit) : (s.flags & ~bit);
        };
        set(input_dtype, srt::kFlagInputFloat16, "input");
        set(output_dtype, srt::kFlagOutputFloat16, "output");
        srt::SaveScene(s, dst_path);
    });
}

ML_API_ENTRY int srtSceneFrame(const char* path, size_t width, size_t height, float* frame12) {
    return Guarded([&] {
        if (path == nullptr || frame12 == nullptr || width == 0 || height == 0) {
            throw std::runtime_error("Bad argument");
        }
        const srt::Frame f = srt::MakeFrame(srt::LoadScene(path).camera, width, height);
        for (int k = 0; k < 3; ++k) {
            frame12[k] = f.origin[k];
            frame12[3 + k] = f.base[k];
            frame12[6 + k] = f.du[k];
            frame12[9 + k] = f.dv[k];
        }
    });
}

ML_API_ENTRY srt_device_scene srtDeviceSceneCreate(const char* path, int device) {
    srt::DeviceScene* out = nullptr;
    Guarded([&] {
        if (path == nullptr) {
            throw std::runtime_error("Bad path argument");
        }
        const srt::Scene scene = srt::LoadScene(path);
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
            throw std::runtime_error("HIP error: device " + std::to_string(device) + " not available (" +
                                     std::to_string(count) + " present); the device stages have no CPU path (ml* renders on the CPU with ML_VISIBLE_DEVICES=cpu)");
        }
        out = new srt::DeviceScene(scene, device);
    });
    return reinterpret_cast<srt_device_scene>(out);
}

ML_API_ENTRY void srtDeviceSceneRelease(srt_device_scene scene) { delete FromHandle(scene); }

ML_API_ENTRY unsigned long long srtDeviceSceneTriangles(srt_device_scene scene) {
    return scene == nullptr ? 0ULL : FromHandle(scene)->triangles();
}

ML_API_ENTRY int srtDeviceSceneOrder(srt_device_scene scene, unsigned* order, unsigned long long capacity,
                                     double* build_ms) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        srt::DeviceScene* s = FromHandle(scene);
        if (order != nullptr) {
            if (capacity < s->triangles()) {
                throw std::runtime_error("Buffer too small: " + std::to_string(capacity) + " entries for " +
                                         std::to_string(s->triangles()));
            }
            Bind bind(s->device());
            srt::HipCheck(hipMemcpy(order, s->order(), s->triangles() * sizeof(unsigned), hipMemcpyDeviceToHost),
                          "hipMemcpy(order)");
        }
        if (build_ms != nullptr) {
            *build_ms = s->build_ms();
        }
    });
}

ML_API_ENTRY int srtPrepareAsync(srt_device_scene scene, size_t width, size_t height, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Prepare(width, height, static_cast<hipStream_t>(stream));
    });
}

ML_API_ENTRY int srtTraceAsync(srt_device_scene scene, const float* d_offsets, float* d_rgba, size_t row_begin,
                               size_t row_count, int variant, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        if ((d_offsets == nullptr || d_rgba == nullptr) && row_count != 0) {
            throw std::runtime_error("Bad buffer argument");
        }
        if (variant != SRT_TRACE_LDS && variant != SRT_TRACE_SCALAR && variant != SRT_TRACE_CULL &&
            variant != SRT_TRACE_BVH) {
            throw std::runtime_error("Unknown trace variant " + std::to_string(variant));
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Trace(d_offsets, d_rgba, row_begin, row_count, variant, static_cast<hipStream_t>(stream));
    });
}

ML_API_ENTRY int srtTraceIdsAsync(srt_device_scene scene, const float* d_offsets, int* d_ids, size_t row_begin,
                                  size_t row_count, int variant, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        if ((d_offsets == nullptr || d_ids == nullptr) && row_count != 0) {
            throw std::runtime_error("Bad buffer argument");
        }
        if (variant != SRT_TRACE_LDS && variant != SRT_TRACE_SCALAR && variant != SRT_TRACE_CULL &&
            variant != SRT_TRACE_BVH) {
            throw std::runtime_error("Unknown trace variant " + std::to_string(variant));
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Trace(d_offsets, nullptr, row_begin, row_count, variant, static_cast<hipStream_t>(stream), d_ids);
    });
}

static_assert(SRT_MAX_BATCH == srt::kMaxBatch, "include/srt_render.h SRT_MAX_BATCH");
static_assert(SRT_TILE_ROWS == srt::kCullTileRows, "include/srt_render.h SRT_TILE_ROWS");

ML_API_ENTRY int srtTraceBatchAsync(srt_device_scene scene, const float* const* d_offsets, float* const* d_rgba,
                                    int* const* d_ids, size_t frames, size_t row_begin, size_t row_count,
                                    size_t row_interleave, int variant, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        if (frames > SRT_MAX_BATCH) {
            throw std::runtime_error("At most " + std::to_string(SRT_MAX_BATCH) + " frames per batch");
        }
        if (frames != 0 && row_count != 0) {
            if (d_offsets == nullptr || (d_rgba == nullptr) == (d_ids == nullptr)) {
                throw std::runtime_error("Bad buffer argument");
            }
            for (size_t f = 0; f < frames; ++f) {
                if (d_offsets[f] == nullptr || (d_rgba != nullptr ? d_rgba[f] == nullptr : d_ids[f] == nullptr)) {
                    throw std::runtime_error("Bad buffer argument");
                }
            }
        }
        if (variant != SRT_TRACE_LDS && variant != SRT_TRACE_SCALAR && variant != SRT_TRACE_CULL &&
            variant != SRT_TRACE_BVH) {
            throw std::runtime_error("Unknown trace variant " + std::to_string(variant));
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->TraceBatch(d_offsets, d_rgba, d_ids, frames, row_begin, row_count, variant, static_cast<hipStream_t>(stream),
                      row_interleave);
    });
}

ML_API_ENTRY int srtShadeAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids, float* d_rgba,
                               size_t row_begin, size_t row_count, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        if ((d_offsets == nullptr || d_ids == nullptr || d_rgba == nullptr) && row_count != 0) {
            throw std::runtime_error("Bad buffer argument");
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Shade(d_offsets, d_ids, d_rgba, row_begin, row_count, static_cast<hipStream_t>(stream));
    });
}

ML_API_ENTRY int srtShadeBandsAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids, float* d_rgba,
                                    size_t frames, size_t band_rows, size_t interleaved, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        if ((d_offsets == nullptr || d_ids == nullptr || d_rgba == nullptr) && frames != 0) {
            throw std::runtime_error("Bad buffer argument");
        }
        if (band_rows == 0) {
            throw std::runtime_error("band_rows must be positive");
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Shade(d_offsets, d_ids, d_rgba, 0, s->height(), static_cast<hipStream_t>(stream), frames, band_rows,
                 interleaved);
    });
}

ML_API_ENTRY int srtSetStageTiming(srt_device_scene scene, int enable) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        FromHandle(scene)->SetTiming(enable != 0);
    });
}

ML_API_ENTRY int srtTakeStageTimes(srt_device_scene scene, unsigned* launches, double* prepare_ms, double* bin_ms,
                                   double* trace_ms) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        const srt::DeviceScene::StageTimes t = s->TakeTimes();
        if (launches != nullptr) {
            *launches = t.launches;
        }
        if (prepare_ms != nullptr) {
            *prepare_ms = t.prepare_ms;
        }
        if (bin_ms != nullptr) {
            *bin_ms = t.bin_ms;
        }
        if (trace_ms != nullptr) {
            *trace_ms = t.kernel_ms;
        }
    });
}

static_assert(SRT_SPLIT_BANDS == srt::EngineOptions::kBands && SRT_SPLIT_FRAMES == srt::EngineOptions::kFrames,
              "include/srt_render.h SRT_SPLIT_*");
static_assert(SRT_EXCHANGE_ALLTOALL == srt::EngineOptions::kAllToAll &&
                  SRT_EXCHANGE_ROTATING == srt::EngineOptions::kRotatingGather &&
                  SRT_EXCHANGE_ROOT == srt::EngineOptions::kRootGather &&
                  SRT_EXCHANGE_SHARE == srt::EngineOptions::kShare,
              "include/srt_render.h SRT_EXCHANGE_*");

}  // extern "C"

namespace {
srt::FrameEngine* FromHandle(srt_engine e) { return reinterpret_cast<srt::FrameEngine*>(e); }

srt::EngineOptions EngineOptionsFrom(const srt_engine_options* o) {
    srt::EngineOptions opt;
    if (o != nullptr) {
        if (o->struct_size != sizeof(srt_engine_options)) {
            throw std::runtime_error("srt_engine_options.struct_size is " + std::to_string(o->struct_size) + ", expected " +
                                     std::to_string(sizeof(srt_engine_options)) + " (a caller built against another "
                                     "include/srt_render.h)");
        }
        opt.variant = o->variant;
        opt.queues = o->queues == 0 ? opt.queues : o->queues;
        opt.batch = o->batch == 0 ? opt.batch : o->batch;
        if (o->rows != SRT_ROWS_INTERLEAVED && o->rows != SRT_ROWS_CONTIGUOUS && o->rows != SRT_ROWS_ROTATED) {
            throw std::runtime_error("Unknown rows mode " + std::to_string(o->rows));
        }
        opt.interleaved = o->rows == SRT_ROWS_INTERLEAVED;
        opt.rotate = o->rows == SRT_ROWS_ROTATED;
        opt.exchange = o->exchange;
        opt.split = o->split;
        opt.simulate = o->simulate != 0;
        opt.launch = o->launch;
        if ((o->flags & ~SRT_ENGINE_RCCL_SELF) != 0) {
            throw std::runtime_error("Unknown engine flags " + std::to_string(o->flags));
        }
        opt.rccl_self = (o->flags & SRT_ENGINE_RCCL_SELF) != 0;
        opt.share = o->share;
        opt.own_rows = o->own_rows;
    }
    return opt;
}

void CheckDevices(const int* devices, std::size_t count) {
    int present = 0;
    if (hipGetDeviceCount(&present) != hipSuccess || present <= 0) {
        throw std::runtime_error("HIP error: no HIP device available; the frame engine has no CPU path (ml* renders on the CPU "
                                 "with ML_VISIBLE_DEVICES=cpu)");
    }
    for (std::size_t i = 0; i < count; ++i) {
        if (devices[i] < 0 || devices[i] >= present) {
            throw std::runtime_error("HIP error: device " + std::to_string(devices[i]) + " not available (" +
                                     std::to_string(present) + " present)");
        }
    }
}
}  // namespace

extern "C" {

ML_API_ENTRY int srtEngineUniqueId(void* id128) {
    return Guarded([&] {
        if (id128 == nullptr) {
            throw std::runtime_error("Bad argument");
        }
        srt::FrameEngine::UniqueId(id128);
    });
}

ML_API_ENTRY srt_engine srtEngineCreate(const char* scene_path, const int* devices, size_t device_count, size_t width,
                                        size_t height, const srt_engine_options* options) {
    srt::FrameEngine* out = nullptr;
    Guarded([&] {
        if (scene_path == nullptr || devices == nullptr || device_count == 0) {
            throw std::runtime_error("Bad argument");
        }
        CheckDevices(devices, device_count);
        const srt::Scene scene = srt::LoadScene(scene_path);
        out = new srt::FrameEngine(scene, std::vector<int>(devices, devices + device_count), width, height,
                                   EngineOptionsFrom(options));
    });
    return reinterpret_cast<srt_engine>(out);
}

ML_API_ENTRY srt_engine srtEngineCreateRank(const char* scene_path, int device, int rank, int world,
                                            const void* unique_id128, size_t width, size_t height,
                                            const srt_engine_options* options) {
    srt::FrameEngine* out = nullptr;
    Guarded([&] {
        if (scene_path == nullptr) {
            throw std::runtime_error("Bad argument");
        }
        CheckDevices(&device, 1);
        const srt::Scene scene = srt::LoadScene(scene_path);
        out = new srt::FrameEngine(scene, device, rank, world, unique_id128, width, height, EngineOptionsFrom(options));
    });
    return reinterpret_cast<srt_engine>(out);
}

ML_API_ENTRY void srtEngineRelease(srt_engine engine) {
    srt::FrameEngine* e = FromHandle(engine);
    if (e != nullptr && e->wedged()) {
        // Deliberately leaked: a device worker never returned from the failed run and still executes
        // inside the engine (its state, communicators' control block and job); freeing any of it
        // would let that thread touch freed memory if its HIP call ever returns (after a GPU reset).
        return;
    }
    delete e;
}

ML_API_ENTRY int srtEngineSetInputs(srt_engine engine, const float* host_offsets, size_t count) {
    return Guarded([&] {
        if (engine == nullptr) {
            throw std::runtime_error("Bad engine handle");
        }
        FromHandle(engine)->SetInputs(host_offsets, count);
    });
}

ML_API_ENTRY int srtEngineRun(srt_engine engine, size_t batches) {
    return Guarded([&] {
        if (engine == nullptr) {
            throw std::runtime_error("Bad engine handle");
        }
        FromHandle(engine)->Run(batches);
    });
}

ML_API_ENTRY int srtEngineVerify(srt_engine engine, size_t* mismatches, size_t* checked) {
    return Guarded([&] {
        if (engine == nullptr) {
            throw std::runtime_error("Bad engine handle");
        }
        const std::size_t bad = FromHandle(engine)->Verify(checked);
        if (mismatches != nullptr) {
            *mismatches = bad;
        }
    });
}

ML_API_ENTRY int srtEngineReadFrame(srt_engine engine, size_t frame, float* host_rgba) {
    return Guarded([&] {
        if (engine == nullptr || host_rgba == nullptr) {
            throw std::runtime_error("Bad argument");
        }
        if (!FromHandle(engine)->ReadFrame(frame, host_rgba)) {
            throw std::runtime_error("Frame " + std::to_string(frame) + " is not resident on this process's devices");
        }
    });
}

ML_API_ENTRY int srtEngineStageTimes(srt_engine engine, size_t local, size_t launches, unsigned* launched,
                                     double* prepare_ms, double* bin_ms, double* trace_ms) {
    return Guarded([&] {
        if (engine == nullptr) {
            throw std::runtime_error("Bad engine handle");
        }
        const srt::DeviceScene::StageTimes t = FromHandle(engine)->MeasureStages(local, launches);
        if (launched != nullptr) {
            *launched = t.launches;
        }
        if (prepare_ms != nullptr) {
            *prepare_ms = t.prepare_ms;
        }
        if (bin_ms != nullptr) {
            *bin_ms = t.bin_ms;
        }
        if (trace_ms != nullptr) {
            *trace_ms = t.kernel_ms;
        }
    });
}

ML_API_ENTRY int srtEngineStageTimesBatch(srt_engine engine, size_t local, size_t launches, size_t frames,
                                          unsigned* launched, double* prepare_ms, double* bin_ms, double* trace_ms) {
    return Guarded([&] {
        if (engine == nullptr) {
            throw std::runtime_error("Bad engine handle");
        }
        const srt::DeviceScene::StageTimes t = FromHandle(engine)->MeasureStages(local, launches, frames);
        if (launched != nullptr) {
            *launched = t.launches;
        }
        if (prepare_ms != nullptr) {
            *prepare_ms = t.prepare_ms;
        }
        if (bin_ms != nullptr) {
            *bin_ms = t.bin_ms;
        }
        if (trace_ms != nullptr) {
            *trace_ms = t.kernel_ms;
        }
    });
}

ML_API_ENTRY int srtEnginePoolSelfTest(size_t workers, size_t failing, int mode, double timeout_s, double* elapsed_s,
                                       int* abort_calls, char* msg, size_t msg_size) {
    return Guarded([&] {
        if (workers == 0 || workers > 64 || failing >= workers || (mode != 1 && mode != 2) || !(timeout_s > 0)) {
            throw std::runtime_error("Bad argument");
        }
        const std::string e = srt::FrameEngine::PoolSelfTest(workers, failing, mode, timeout_s, elapsed_s, abort_calls);
        if (msg != nullptr && msg_size != 0) {
            const std::size_t n = std::min(e.size(), msg_size - 1);
            std::memcpy(msg, e.data(), n);
            msg[n] = '\0';
        }
    });
}

ML_API_ENTRY size_t srtShareAuto(size_t height, size_t devices) {
    return srt::ShareAuto(height, devices);
}

ML_API_ENTRY size_t srtRotateOwnRows(size_t height) {
    size_t rows = 0;
    (void)Guarded([&] { rows = srt::RotateOwnRows(height); });  // 0: SRT_ROTATE_OWN invalid (srtGetLastError)
    return rows;
}

ML_API_ENTRY size_t srtRotateSplitForLink(size_t height, size_t width, double link_gbs, double frame_us,
                                          double bytes_per_pixel) {
    return srt::RotateSplitForLink(height, width, link_gbs, frame_us, bytes_per_pixel);
}

ML_API_ENTRY int srtEngineSplit(srt_engine engine, size_t* own_rows, size_t* buffer_rows, double* link_gbs,
                                double* frame_us, int* source) {
    return Guarded([&] {
        if (engine == nullptr) {
            throw std::runtime_error("Bad engine handle");
        }
        const srt::FrameEngine::SplitInfo s = FromHandle(engine)->split_info();
        if (own_rows != nullptr) {
            *own_rows = s.own_rows;
        }
        if (buffer_rows != nullptr) {
            *buffer_rows = s.buffer_rows;
        }
        if (link_gbs != nullptr) {
            *link_gbs = s.link_gbs;
        }
        if (frame_us != nullptr) {
            *frame_us = s.frame_us;
        }
        if (source != nullptr) {
            *source = s.source;
        }
    });
}

ML_API_ENTRY int srtEngineInfo(srt_engine engine, size_t* devices, size_t* local_devices, size_t* band_rows,
                               size_t* buffer_rows, int* rccl, double* exchange_bytes_per_frame) {
    return Guarded([&] {
        if (engine == nullptr) {
            throw std::runtime_error("Bad engine handle");
        }
        const srt::FrameEngine* e = FromHandle(engine);
        if (devices != nullptr) {
            *devices = e->devices();
        }
        if (local_devices != nullptr) {
            *local_devices = e->local_devices();
        }
        if (band_rows != nullptr) {
            *band_rows = e->band_rows(0);
        }
        if (buffer_rows != nullptr) {
            *buffer_rows = e->buffer_rows();
        }
        if (rccl != nullptr) {
            *rccl = e->uses_rccl() ? 1 : 0;
        }
        if (exchange_bytes_per_frame != nullptr) {
            *exchange_bytes_per_frame = e->exchange_bytes_per_frame();
        }
    });
}

ML_API_ENTRY int srtEngineExchangeStats(srt_engine engine, size_t local, size_t* groups, double* ms_mean,
                                        double* bytes_sent) {
    return Guarded([&] {
        if (engine == nullptr) {
            throw std::runtime_error("Bad engine handle");
        }
        const srt::FrameEngine* e = FromHandle(engine);
        if (local >= e->local_devices()) {
            throw std::runtime_error("srtEngineExchangeStats: no local device " + std::to_string(local));
        }
        const srt::FrameEngine::ExchangeStats st = e->exchange_stats(local);
        if (groups != nullptr) {
            *groups = st.groups;
        }
        if (ms_mean != nullptr) {
            *ms_mean = st.ms_mean;
        }
        if (bytes_sent != nullptr) {
            *bytes_sent = st.bytes_sent;
        }
    });
}

namespace {
int ExchangeHost(const int* const* band_ids, size_t bands, size_t width, size_t height, int rows, int exchange,
                 size_t share, size_t batch, size_t batch_index, int* const* recv, size_t* recv_frames,
                 size_t* buffer_rows) {
    return Guarded([&] {
        if (bands == 0 || width == 0 || height == 0 || batch == 0 ||
            (rows != SRT_ROWS_INTERLEAVED && rows != SRT_ROWS_CONTIGUOUS && rows != SRT_ROWS_ROTATED) ||
            exchange < SRT_EXCHANGE_ALLTOALL || exchange > SRT_EXCHANGE_SHARE ||
            (rows == SRT_ROWS_ROTATED && exchange != SRT_EXCHANGE_ALLTOALL) ||
            (exchange == SRT_EXCHANGE_SHARE && (rows != SRT_ROWS_INTERLEAVED || bands < 2))) {
            throw std::runtime_error("Bad argument");
        }
        if (exchange == SRT_EXCHANGE_SHARE) {
            share = share == 0 ? srt::ShareAuto(height, bands) : share;
            if (share > 64 || (share & (share - 1)) != 0) {
                throw std::runtime_error("share must be a power of two, 1..64");
            }
        }
        // The engine's layout (EngineSplit: kShare splits the frame into share + P - 1 interleaved classes;
        // rotated over two devices band 0 takes the split an engine without a measured link uses,
        // RotateOwnRows -- env SRT_ROTATE_OWN, default 80 %)
        const srt::BandSplit split =
            srt::EngineSplit(height, bands, true, rows == SRT_ROWS_INTERLEAVED, rows == SRT_ROWS_ROTATED,
                             exchange == SRT_EXCHANGE_SHARE ? share : 0, 0);
        srt::ExchangePlan plan;
        plan.bands = bands;
        plan.batch = batch;
        plan.exchange = exchange;
        plan.rotate = rows == SRT_ROWS_ROTATED && bands > 1;
        if (buffer_rows != nullptr) {
            *buffer_rows = split.BufferRows();
        }
        if (recv_frames != nullptr) {
            for (size_t c = 0; c < bands; ++c) {
                recv_frames[c] = plan.FramesFor(batch_index, c);
            }
        }
        if (recv == nullptr) {
            return;
        }
        if (band_ids == nullptr) {
            throw std::runtime_error("Bad argument");
        }
        const size_t pixels = batch * split.BufferRows() * width;
        std::vector<std::vector<int>> in(bands);
        for (size_t d = 0; d < bands; ++d) {
            in[d].assign(band_ids[d], band_ids[d] + pixels);
        }
        const std::vector<std::vector<int>> out = srt::ExchangeOnHost(split, plan, width, batch_index, in);
        for (size_t c = 0; c < bands; ++c) {
            if (!out[c].empty()) {
                std::copy(out[c].begin(), out[c].end(), recv[c]);
            }
        }
    });
}
}  // namespace

ML_API_ENTRY int srtExchangeHost(const int* const* band_ids, size_t bands, size_t width, size_t height, int rows,
                                 int exchange, size_t batch, size_t batch_index, int* const* recv,
                                 size_t* recv_frames, size_t* buffer_rows) {
    if (exchange == SRT_EXCHANGE_SHARE) {  // needs its share parameter: srtExchangeHostShare
        return Guarded([] { throw std::runtime_error("Bad argument: the share exchange takes srtExchangeHostShare"); });
    }
    return ExchangeHost(band_ids, bands, width, height, rows, exchange, 0, batch, batch_index, recv, recv_frames,
                        buffer_rows);
}

ML_API_ENTRY int srtExchangeHostShare(const int* const* band_ids, size_t bands, size_t width, size_t height,
                                      size_t share, size_t batch, size_t batch_index, int* const* recv,
                                      size_t* recv_frames, size_t* buffer_rows) {
    return ExchangeHost(band_ids, bands, width, height, SRT_ROWS_INTERLEAVED, SRT_EXCHANGE_SHARE, share, batch,
                        batch_index, recv, recv_frames, buffer_rows);
}

ML_API_ENTRY int srtScreenBoxHost(const float* c, int mode, float* box) {
    return Guarded([&] {
        if (c == nullptr || box == nullptr || mode < 0 || mode > 2) {
            throw std::runtime_error("Bad argument");
        }
        if (!srt::HostScreenBox(c, mode, box)) {
            throw std::runtime_error("screen box: the float fast path does not apply");
        }
    });
}

// Point queries (include/srt_query.h): the rtq family.
RTQ_API int rtqQueryAsync(srt_device_scene scene, const float* d_positions, size_t count, int* d_ids, float* d_t,
                          unsigned char* d_how, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        if (count != 0) {
            if (d_positions == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_positions is NULL");
            }
            if (d_ids == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_ids is NULL");
            }
            if (d_t == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_t is NULL");
            }
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Query(d_positions, count, d_ids, d_t, d_how, static_cast<hipStream_t>(stream));
    });
}

RTQ_API int rtqQueryHost(const char* scene_path, size_t width, size_t height, const float* positions, size_t count,
                         int* ids, float* t) {
    return Guarded([&] {
        if (scene_path == nullptr || width == 0 || height == 0 ||
            (count != 0 && (positions == nullptr || ids == nullptr || t == nullptr))) {
            throw std::runtime_error("Bad argument");
        }
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostClosestHits(scene, width, height, positions, count, ids, t);
    });
}

RTQ_API int rtqTileHost(size_t width, size_t height, float fx, float fy, int* tile_col, int* tile_row) {
    return Guarded([&] {
        if (tile_col == nullptr || tile_row == nullptr || width == 0 || height == 0 ||
            !srt::CullBinnable(width, height)) {
            throw std::runtime_error("Bad argument");
        }
        const int nx = static_cast<int>((width + srt::kCullTileCols - 1) / srt::kCullTileCols);
        const int ny = static_cast<int>((height + srt::kCullTileRows - 1) / srt::kCullTileRows);
        if (!srt::TileOfPosition(fx, fy, static_cast<float>(width), static_cast<float>(height), srt::kCullTileCols,
                                 srt::kCullTileRows, nx, ny, *tile_col, *tile_row)) {
            throw std::runtime_error("Position outside [0, 1]^2: no tile");
        }
    });
}

// G-buffer outputs (include/srt_gbuffer.h): the rtg family.
namespace {

rtg_outputs CheckedOutputs(const rtg_outputs* o) {
    if (o == nullptr) {
        throw std::runtime_error("Bad argument: outputs is NULL");
    }
    if (o->struct_size != sizeof(rtg_outputs)) {
        throw std::runtime_error("rtg_outputs.struct_size is " + std::to_string(o->struct_size) + ", expected " +
                                 std::to_string(sizeof(rtg_outputs)));
    }
    return *o;
}

bool NoPlane(const rtg_outputs& o) {
    return o.depth == nullptr && o.bary == nullptr && o.normal == nullptr && o.albedo == nullptr;
}

}  // namespace

RTG_API int rtgFrameAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids, size_t row_begin,
                          size_t row_count, const rtg_outputs* outputs, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        const rtg_outputs o = CheckedOutputs(outputs);
        if (row_count != 0 && !NoPlane(o)) {
            if (d_offsets == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_offsets is NULL");
            }
            if (d_ids == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_ids is NULL");
            }
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->GBuffer(false, d_offsets, d_ids, row_begin, row_count, o.depth, o.bary, o.normal, o.albedo,
                   static_cast<hipStream_t>(stream));
    });
}

RTG_API int rtgPointsAsync(srt_device_scene scene, const float* d_positions, const int* d_ids, size_t count,
                           const rtg_outputs* outputs, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        const rtg_outputs o = CheckedOutputs(outputs);
        if (count != 0 && !NoPlane(o)) {
            if (d_positions == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_positions is NULL");
            }
            if (d_ids == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_ids is NULL");
            }
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->GBuffer(true, d_positions, d_ids, 0, count, o.depth, o.bary, o.normal, o.albedo,
                   static_cast<hipStream_t>(stream));
    });
}

RTG_API int rtgPointsHost(const char* scene_path, size_t width, size_t height, const float* positions,
                          const int* ids, size_t count, const rtg_outputs* outputs) {
    return Guarded([&] {
        const rtg_outputs o = CheckedOutputs(outputs);
        if (scene_path == nullptr || width == 0 || height == 0 ||
            (count != 0 && !NoPlane(o) && (positions == nullptr || ids == nullptr))) {
            throw std::runtime_error("Bad argument");
        }
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostGBuffer(scene, width, height, positions, ids, count, o.depth, o.bary, o.normal, o.albedo);
    });
}

// Multi-sample frames (include/srt_samples.h): the rts family.
static_assert(RTS_MAX_SAMPLES == srt::kMaxSamples, "include/srt_samples.h RTS_MAX_SAMPLES");

namespace {

void CheckSamples(size_t samples) {
    if (samples == 0 || samples > RTS_MAX_SAMPLES) {
        throw std::runtime_error("Bad argument: samples must be 1 to " + std::to_string(RTS_MAX_SAMPLES) + ", got " +
                                 std::to_string(samples));
    }
}

// The plane pointer arrays and the output of a call that has pixels to resolve.
void CheckPlanes(const char* offsets_name, const float* const* offsets, const char* ids_name, const int* const* ids,
                 size_t samples, const char* rgba_name, const float* rgba) {
    if (offsets == nullptr) {
        throw std::runtime_error(std::string("Bad buffer argument: ") + offsets_name + " is NULL");
    }
    if (ids == nullptr) {
        throw std::runtime_error(std::string("Bad buffer argument: ") + ids_name + " is NULL");
    }
    for (size_t s = 0; s < samples; ++s) {
        if (offsets[s] == nullptr) {
            throw std::runtime_error(std::string("Bad buffer argument: ") + offsets_name + "[" + std::to_string(s) +
                                     "] is NULL");
        }
        if (ids[s] == nullptr) {
            throw std::runtime_error(std::string("Bad buffer argument: ") + ids_name + "[" + std::to_string(s) +
                                     "] is NULL");
        }
    }
    if (rgba == nullptr) {
        throw std::runtime_error(std::string("Bad buffer argument: ") + rgba_name + " is NULL");
    }
}

}  // namespace

RTS_API int rtsResolveAsync(srt_device_scene scene, const float* const* d_offsets, const int* const* d_ids,
                            size_t samples, size_t row_begin, size_t row_count, float* d_rgba, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        CheckSamples(samples);
        if (row_count != 0) {
            CheckPlanes("d_offsets", d_offsets, "d_ids", d_ids, samples, "d_rgba", d_rgba);
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Resolve(d_offsets, d_ids, samples, row_begin, row_count, d_rgba, static_cast<hipStream_t>(stream));
    });
}

RTS_API int rtsRenderAsync(srt_device_scene scene, const float* const* d_offsets, int* const* d_ids, size_t samples,
                           float* d_rgba, int variant, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        CheckSamples(samples);
        srt::DeviceScene* s = FromHandle(scene);
        if (s->width() == 0) {
            throw std::runtime_error("RenderSamples: Prepare() has not been called");
        }
        CheckPlanes("d_offsets", d_offsets, "d_ids", d_ids, samples, "d_rgba", d_rgba);
        if (variant != SRT_TRACE_LDS && variant != SRT_TRACE_SCALAR && variant != SRT_TRACE_CULL &&
            variant != SRT_TRACE_BVH) {
            throw std::runtime_error("Unknown trace variant " + std::to_string(variant));
        }
        Bind bind(s->device());
        s->RenderSamples(d_offsets, d_ids, samples, d_rgba, variant, static_cast<hipStream_t>(stream));
    });
}

RTS_API int rtsResolveHost(const char* scene_path, size_t width, size_t height, const float* const* offsets,
                           const int* const* ids, size_t samples, size_t row_begin, size_t row_count, float* rgba) {
    return Guarded([&] {
        if (scene_path == nullptr) {
            throw std::runtime_error("Bad argument: scene_path is NULL");
        }
        if (width == 0 || height == 0) {
            throw std::runtime_error("Bad argument: width and height must be non-zero");
        }
        CheckSamples(samples);
        if (row_begin > height || row_count > height - row_begin) {
            throw std::runtime_error("Bad argument: row band outside the frame");
        }
        if (row_count == 0) {
            return;
        }
        CheckPlanes("offsets", offsets, "ids", ids, samples, "rgba", rgba);
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostResolve(scene, width, height, offsets, ids, samples, row_begin, row_count, rgba);
    });
}

// Depth layers (include/srt_layers.h): the rtk family.
static_assert(RTK_MAX_LAYERS == srt::kMaxLayers, "include/srt_layers.h RTK_MAX_LAYERS");

namespace {

void CheckLayers(size_t layers) {
    if (layers == 0 || layers > RTK_MAX_LAYERS) {
        throw std::runtime_error("Bad argument: layers must be 1 to " + std::to_string(RTK_MAX_LAYERS) + ", got " +
                                 std::to_string(layers));
    }
}

void CheckBuffer(const char* name, const void* p) {
    if (p == nullptr) {
        throw std::runtime_error(std::string("Bad buffer argument: ") + name + " is NULL");
    }
}

}  // namespace

RTK_API int rtkLayersAsync(srt_device_scene scene, const float* d_positions, size_t count, size_t layers, int* d_ids,
                           float* d_t, unsigned char* d_how, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        CheckLayers(layers);
        if (count != 0) {
            CheckBuffer("d_positions", d_positions);
            CheckBuffer("d_ids", d_ids);
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Layers(true, d_positions, 0, count, layers, d_ids, d_t, d_how, static_cast<hipStream_t>(stream));
    });
}

RTK_API int rtkFrameAsync(srt_device_scene scene, const float* d_offsets, size_t row_begin, size_t row_count,
                          size_t layers, int* d_ids, float* d_t, unsigned char* d_how, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        CheckLayers(layers);
        if (row_count != 0) {
            CheckBuffer("d_offsets", d_offsets);
            CheckBuffer("d_ids", d_ids);
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Layers(false, d_offsets, row_begin, row_count, layers, d_ids, d_t, d_how, static_cast<hipStream_t>(stream));
    });
}

RTK_API int rtkCompositeAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids, size_t layers,
                              const float* d_opacity, size_t row_begin, size_t row_count, float* d_rgba, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        CheckLayers(layers);
        if (row_count != 0) {
            CheckBuffer("d_offsets", d_offsets);
            CheckBuffer("d_ids", d_ids);
            CheckBuffer("d_opacity", d_opacity);
            CheckBuffer("d_rgba", d_rgba);
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Composite(d_offsets, d_ids, layers, d_opacity, row_begin, row_count, d_rgba, static_cast<hipStream_t>(stream));
    });
}

RTK_API int rtkLayersHost(const char* scene_path, size_t width, size_t height, const float* positions, size_t count,
                          size_t layers, int* ids, float* t) {
    return Guarded([&] {
        if (scene_path == nullptr) {
            throw std::runtime_error("Bad argument: scene_path is NULL");
        }
        if (width == 0 || height == 0) {
            throw std::runtime_error("Bad argument: width and height must be non-zero");
        }
        CheckLayers(layers);
        if (count == 0) {
            return;
        }
        CheckBuffer("positions", positions);
        CheckBuffer("ids", ids);
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostLayers(scene, width, height, positions, count, layers, ids, t);
    });
}

RTK_API int rtkCompositeHost(const char* scene_path, size_t width, size_t height, const float* offsets, const int* ids,
                             size_t layers, const float* opacity, size_t row_begin, size_t row_count, float* rgba) {
    return Guarded([&] {
        if (scene_path == nullptr) {
            throw std::runtime_error("Bad argument: scene_path is NULL");
        }
        if (width == 0 || height == 0) {
            throw std::runtime_error("Bad argument: width and height must be non-zero");
        }
        CheckLayers(layers);
        if (row_begin > height || row_count > height - row_begin) {
            throw std::runtime_error("Bad argument: row band outside the frame");
        }
        if (row_count == 0) {
            return;
        }
        CheckBuffer("offsets", offsets);
        CheckBuffer("ids", ids);
        CheckBuffer("opacity", opacity);
        CheckBuffer("rgba", rgba);
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostComposite(scene, width, height, offsets, ids, layers, opacity, row_begin, row_count, rgba);
    });
}

// Spot-light shadow masks (include/srt_light.h): the rtl family.
using srt::CheckedCamera;  // scene.h: shared with the rtm family below

RTL_API srt_device_scene rtlSceneCreate(const char* path, int device, const float camera10[10]) {
    srt::DeviceScene* out = nullptr;
    Guarded([&] {
        if (path == nullptr) {
            throw std::runtime_error("Bad path argument");
        }
        srt::Scene scene = srt::LoadScene(path);
        if (camera10 != nullptr) {
            scene.camera = CheckedCamera(camera10);
        }
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
            throw std::runtime_error("HIP error: device " + std::to_string(device) + " not available (" +
                                     std::to_string(count) + " present); the device stages have no CPU path");
        }
        out = new srt::DeviceScene(scene, device);
    });
    return reinterpret_cast<srt_device_scene>(out);
}

RTL_API int rtlShadowAsync(srt_device_scene view, srt_device_scene light, const float* d_offsets, const int* d_ids,
                           size_t row_begin, size_t row_count, float bias, unsigned char* d_mask, float* d_rgba,
                           float dim, void* stream) {
    return Guarded([&] {
        if (view == nullptr) {
            throw std::runtime_error("Bad scene handle: view is NULL");
        }
        if (light == nullptr) {
            throw std::runtime_error("Bad scene handle: light is NULL");
        }
        if (row_count != 0) {
            if (d_offsets == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_offsets is NULL");
            }
            if (d_ids == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_ids is NULL");
            }
            if (d_mask == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_mask is NULL");
            }
        }
        srt::DeviceScene* s = FromHandle(view);
        Bind bind(s->device());
        s->Shadow(*FromHandle(light), d_offsets, d_ids, row_begin, row_count, bias, d_mask, d_rgba, dim,
                  static_cast<hipStream_t>(stream));
    });
}

RTL_API int rtlShadowHost(const char* scene_path, size_t width, size_t height, const float light_camera10[10],
                          size_t light_width, size_t light_height, const float* offsets, const int* ids,
                          size_t row_begin, size_t row_count, float bias, unsigned char* mask, float* rgba, float dim) {
    return Guarded([&] {
        if (scene_path == nullptr) {
            throw std::runtime_error("Bad argument: scene_path is NULL");
        }
        if (light_camera10 == nullptr) {
            throw std::runtime_error("Bad argument: light_camera10 is NULL");
        }
        if (width == 0 || height == 0 || light_width == 0 || light_height == 0) {
            throw std::runtime_error("Bad argument: frame dimensions must be non-zero");
        }
        const srt::Camera lc = CheckedCamera(light_camera10);
        if (!(bias >= 0.f) || !std::isfinite(bias)) {
            throw std::runtime_error("Shadow: bias must be finite and >= 0");
        }
        if (!std::isfinite(dim)) {
            throw std::runtime_error("Shadow: dim must be finite");
        }
        if (row_begin > height || row_count > height - row_begin) {
            throw std::runtime_error("Bad argument: row band outside the frame");
        }
        if (row_count == 0) {
            return;
        }
        if (offsets == nullptr) {
            throw std::runtime_error("Bad buffer argument: offsets is NULL");
        }
        if (ids == nullptr) {
            throw std::runtime_error("Bad buffer argument: ids is NULL");
        }
        if (mask == nullptr) {
            throw std::runtime_error("Bad buffer argument: mask is NULL");
        }
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostShadow(scene, width, height, lc, light_width, light_height, offsets, ids, row_begin, row_count, bias,
                        mask, rgba, dim);
    });
}

RTL_API int rtlProjectionHost(const float camera10[10], size_t light_width, size_t light_height, float rows9[9]) {
    return Guarded([&] {
        if (camera10 == nullptr || rows9 == nullptr) {
            throw std::runtime_error("Bad argument");
        }
        if (light_width == 0 || light_height == 0) {
            throw std::runtime_error("Bad argument: frame dimensions must be non-zero");
        }
        srt::HostShadowRows(CheckedCamera(camera10), light_width, light_height, rows9);
    });
}

// Omni-light shadow masks (include/srt_omni.h): the rto family.
struct rto_light_t {
    std::unique_ptr<srt::DeviceScene> faces[srt::kOmniFaces];
    int device = 0;
};

namespace {

void CheckedOrigin(const float origin[3]) {
    if (origin == nullptr) {
        throw std::runtime_error("Bad argument: origin is NULL");
    }
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(origin[k]) || std::fabs(origin[k]) > srt::kOmniOriginMax) {
            throw std::runtime_error("Bad light origin: value " + std::to_string(k) +
                                     " must be finite and at most 2^16 in magnitude");
        }
    }
}

void CheckedFace(int face) {
    if (face < 0 || face >= srt::kOmniFaces) {
        throw std::runtime_error("Bad face index " + std::to_string(face) + ": faces are 0 to 5");
    }
}

}  // namespace

RTO_API rto_light rtoLightCreate(const char* path, int device, const float origin[3]) {
    rto_light out = nullptr;
    Guarded([&] {
        if (path == nullptr) {
            throw std::runtime_error("Bad path argument");
        }
        CheckedOrigin(origin);
        srt::Scene scene = srt::LoadScene(path);
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
            throw std::runtime_error("HIP error: device " + std::to_string(device) + " not available (" +
                                     std::to_string(count) + " present); the device stages have no CPU path");
        }
        auto light = std::make_unique<rto_light_t>();
        light->device = device;
        for (int k = 0; k < srt::kOmniFaces; ++k) {
            float c10[10];
            srt::OmniFaceCamera(origin, k, c10);
            scene.camera = CheckedCamera(c10);
            light->faces[k] = std::make_unique<srt::DeviceScene>(scene, device);
        }
        out = light.release();
    });
    return out;
}

RTO_API void rtoLightRelease(rto_light light) { delete light; }

RTO_API int rtoLightPrepareAsync(rto_light light, size_t face_size, void* stream) {
    return Guarded([&] {
        if (light == nullptr) {
            throw std::runtime_error("Bad light handle");
        }
        if (face_size == 0) {
            throw std::runtime_error("Bad argument: face_size must be non-zero");
        }
        Bind bind(light->device);
        for (auto& f : light->faces) {
            f->Prepare(face_size, face_size, static_cast<hipStream_t>(stream));
        }
    });
}

RTO_API srt_device_scene rtoLightFace(rto_light light, int face) {
    srt_device_scene out = nullptr;
    Guarded([&] {
        if (light == nullptr) {
            throw std::runtime_error("Bad light handle");
        }
        CheckedFace(face);
        out = reinterpret_cast<srt_device_scene>(light->faces[face].get());
    });
    return out;
}

RTO_API int rtoShadowAsync(srt_device_scene view, rto_light light, const float* d_offsets, const int* d_ids,
                           size_t row_begin, size_t row_count, float bias, unsigned char* d_mask,
                           unsigned char* d_face, float* d_rgba, float dim, void* stream) {
    return Guarded([&] {
        if (view == nullptr) {
            throw std::runtime_error("Bad scene handle: view is NULL");
        }
        if (light == nullptr) {
            throw std::runtime_error("Bad light handle");
        }
        if (row_count != 0) {
            if (d_offsets == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_offsets is NULL");
            }
            if (d_ids == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_ids is NULL");
            }
            if (d_mask == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_mask is NULL");
            }
        }
        srt::DeviceScene* s = FromHandle(view);
        Bind bind(s->device());
        const srt::DeviceScene* faces[srt::kOmniFaces];
        for (int k = 0; k < srt::kOmniFaces; ++k) {
            faces[k] = light->faces[k].get();
        }
        s->OmniShadow(faces, d_offsets, d_ids, row_begin, row_count, bias, d_mask, d_face, d_rgba, dim,
                      static_cast<hipStream_t>(stream));
    });
}

RTO_API int rtoShadowHost(const char* scene_path, size_t width, size_t height, const float origin[3], size_t face_size,
                          const float* offsets, const int* ids, size_t row_begin, size_t row_count, float bias,
                          unsigned char* mask, unsigned char* face, float* rgba, float dim) {
    return Guarded([&] {
        if (scene_path == nullptr) {
            throw std::runtime_error("Bad argument: scene_path is NULL");
        }
        CheckedOrigin(origin);
        if (width == 0 || height == 0) {
            throw std::runtime_error("Bad argument: frame dimensions must be non-zero");
        }
        if (face_size == 0) {
            throw std::runtime_error("Bad argument: face_size must be non-zero");
        }
        if (!(bias >= 0.f) || !std::isfinite(bias)) {
            throw std::runtime_error("Omni shadow: bias must be finite and >= 0");
        }
        if (!std::isfinite(dim)) {
            throw std::runtime_error("Omni shadow: dim must be finite");
        }
        if (row_begin > height || row_count > height - row_begin) {
            throw std::runtime_error("Bad argument: row band outside the frame");
        }
        if (row_count == 0) {
            return;
        }
        if (offsets == nullptr) {
            throw std::runtime_error("Bad buffer argument: offsets is NULL");
        }
        if (ids == nullptr) {
            throw std::runtime_error("Bad buffer argument: ids is NULL");
        }
        if (mask == nullptr) {
            throw std::runtime_error("Bad buffer argument: mask is NULL");
        }
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostOmniShadow(scene, width, height, origin, face_size, offsets, ids, row_begin, row_count, bias, mask,
                            face, rgba, dim);
    });
}

RTO_API int rtoFaceCameraHost(const float origin[3], int face, float camera10[10]) {
    return Guarded([&] {
        CheckedOrigin(origin);
        CheckedFace(face);
        if (camera10 == nullptr) {
            throw std::runtime_error("Bad argument: camera10 is NULL");
        }
        srt::OmniFaceCamera(origin, face, camera10);
    });
}

RTO_API int rtoFaceOfHost(const float q[3]) {
    int face = -1;
    Guarded([&] {
        if (q == nullptr) {
            throw std::runtime_error("Bad argument: q is NULL");
        }
        face = srt::OmniFace(q);
    });
    return face;
}

// Direct lighting (include/srt_lighting.h): the rtd family. The entry points check what is theirs --
// NULL arguments, the structs' sizes and handles, the host lights' geometry; every rule about the
// lights themselves (count, frame total, ambient, colour, falloff, bias, and for device lights
// preparation, device, triangle count and record source) is DeviceScene's (renderer.cpp).
static_assert(RTD_MAX_LIGHTS == srt::kLightingMaxLights && RTD_MAX_FRAMES == srt::kLightingMaxFrames,
              "include/srt_lighting.h and lighting_math.h agree");

namespace {

// The device lights of a call as DeviceScene takes them (rtdLightAsync, rtpLightSurfaceAsync,
// rthLightHitsAsync): `in` holds count lights, `scenes` count x 6 scene pointers.
void CollectDeviceLights(const rtd_light* lights, size_t count, srt::DeviceScene::Light* in,
                         const srt::DeviceScene** scenes) {
    for (size_t l = 0; l < count; ++l) {
        const rtd_light& lt = lights[l];
        const std::string who = "Lighting: light " + std::to_string(l);
        if (lt.struct_size != sizeof(rtd_light)) {
            throw std::runtime_error(who + ": rtd_light.struct_size is " + std::to_string(lt.struct_size) +
                                     ", expected " + std::to_string(sizeof(rtd_light)));
        }
        if ((lt.spot != nullptr) == (lt.point != nullptr)) {
            throw std::runtime_error(who + ": exactly one of spot and point must be set, got " +
                                     (lt.spot != nullptr ? "both" : "neither"));
        }
        const srt::DeviceScene** mine = scenes + l * srt::kOmniFaces;
        const bool point = lt.point != nullptr;
        for (int k = 0; k < (point ? srt::kOmniFaces : 1); ++k) {
            mine[k] = point ? lt.point->faces[k].get() : FromHandle(lt.spot);
        }
        in[l] = srt::DeviceScene::Light{mine, point, {lt.color[0], lt.color[1], lt.color[2]}, lt.falloff, lt.bias};
    }
}

// The host lights of a call, checked (rtdLightHost, rtpLightSurfaceHost, rthLightHitsHost): the
// structs, DeviceScene::CheckLights' rules with the ambient colour, then each light's geometry.
void CollectHostLights(const rtd_light_host* lights, size_t count, const float ambient[3],
                       std::vector<srt::HostLight>& in) {
    std::vector<srt::DeviceScene::LightTerms> terms(count);
    for (size_t l = 0; l < count; ++l) {
        const rtd_light_host& lt = lights[l];
        const std::string who = "Lighting: light " + std::to_string(l);
        if (lt.struct_size != sizeof(rtd_light_host)) {
            throw std::runtime_error(who + ": rtd_light_host.struct_size is " + std::to_string(lt.struct_size) +
                                     ", expected " + std::to_string(sizeof(rtd_light_host)));
        }
        if (lt.kind != 0 && lt.kind != 1) {
            throw std::runtime_error(who + ": kind must be 0 (spot) or 1 (point), got " + std::to_string(lt.kind));
        }
        terms[l] = srt::DeviceScene::LightTerms{lt.kind == 1, lt.color, lt.falloff, lt.bias};
    }
    srt::DeviceScene::CheckLights(terms.data(), count, ambient);
    in.assign(count, srt::HostLight{});
    for (size_t l = 0; l < count; ++l) {
        const rtd_light_host& lt = lights[l];
        srt::HostLight& h = in[l];
        h = srt::HostLight{};
        h.point = lt.kind == 1;
        try {
            if (h.point) {
                CheckedOrigin(lt.origin);
                if (lt.face_size == 0) {
                    throw std::runtime_error("face_size must be non-zero");
                }
                std::copy(lt.origin, lt.origin + 3, h.origin);
                h.face_size = lt.face_size;
            } else {
                if (lt.width == 0 || lt.height == 0) {
                    throw std::runtime_error("frame dimensions must be non-zero");
                }
                h.camera = CheckedCamera(lt.camera10);
                h.width = lt.width;
                h.height = lt.height;
            }
        } catch (std::exception& e) {
            throw std::runtime_error("Lighting: light " + std::to_string(l) + ": " + e.what());
        }
        std::copy(lt.color, lt.color + 3, h.color);
        h.falloff = lt.falloff;
        h.bias = lt.bias;
    }
}

// rtdLightAsync, and with a `surface` (checked by the caller) rtpLightSurfaceAsync.
int LightAsync(srt_device_scene view, const rtd_light* lights, size_t count, const float ambient[3],
               const srt::LitSurface* surface, const float* d_offsets, const int* d_ids, size_t row_begin,
               size_t row_count, float* d_rgba, unsigned char* d_classes, void* stream) {
    return Guarded([&] {
        if (view == nullptr) {
            throw std::runtime_error("Bad scene handle: view is NULL");
        }
        srt::DeviceScene::CheckLightCount(count);
        if (count != 0 && lights == nullptr) {
            throw std::runtime_error("Bad argument: lights is NULL");
        }
        if (ambient == nullptr) {
            throw std::runtime_error("Bad argument: ambient is NULL");
        }
        std::vector<srt::DeviceScene::Light> in(count);
        std::vector<const srt::DeviceScene*> scenes(count * srt::kOmniFaces);
        CollectDeviceLights(lights, count, in.data(), scenes.data());
        if (row_count != 0) {
            if (d_offsets == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_offsets is NULL");
            }
            if (d_ids == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_ids is NULL");
            }
            if (d_rgba == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_rgba is NULL");
            }
        }
        srt::DeviceScene* s = FromHandle(view);
        Bind bind(s->device());
        if (surface != nullptr) {
            s->LitSurface(in.data(), count, ambient, *surface, d_offsets, d_ids, row_begin, row_count, d_rgba, d_classes,
                          static_cast<hipStream_t>(stream));
        } else {
            s->Lighting(in.data(), count, ambient, d_offsets, d_ids, row_begin, row_count, d_rgba, d_classes,
                        static_cast<hipStream_t>(stream));
        }
    });
}

// rtdLightHost, and with `surface` / `material` (checked by the caller) rtpLightSurfaceHost.
int LightHost(const char* scene_path, size_t width, size_t height, const rtd_light_host* lights, size_t count,
              const float ambient[3], const srt::HostSurfaceTables* surface, const srt::HostMaterial* material,
              const float* offsets, const int* ids, size_t row_begin, size_t row_count, float* rgba,
              unsigned char* classes) {
    return Guarded([&] {
        if (scene_path == nullptr) {
            throw std::runtime_error("Bad argument: scene_path is NULL");
        }
        if (width == 0 || height == 0) {
            throw std::runtime_error("Bad argument: frame dimensions must be non-zero");
        }
        srt::DeviceScene::CheckLightCount(count);
        if (count != 0 && lights == nullptr) {
            throw std::runtime_error("Bad argument: lights is NULL");
        }
        if (ambient == nullptr) {
            throw std::runtime_error("Bad argument: ambient is NULL");
        }
        std::vector<srt::HostLight> in;
        CollectHostLights(lights, count, ambient, in);
        if (row_begin > height || row_count > height - row_begin) {
            throw std::runtime_error("Bad argument: row band outside the frame");
        }
        if (row_count == 0) {
            return;
        }
        if (offsets == nullptr) {
            throw std::runtime_error("Bad buffer argument: offsets is NULL");
        }
        if (ids == nullptr) {
            throw std::runtime_error("Bad buffer argument: ids is NULL");
        }
        if (rgba == nullptr) {
            throw std::runtime_error("Bad buffer argument: rgba is NULL");
        }
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostLitSurface(scene, width, height, in.data(), count, ambient, surface, material, offsets, ids, row_begin,
                            row_count, rgba, classes);
    });
}

}  // namespace

RTD_API int rtdLightAsync(srt_device_scene view, const rtd_light* lights, size_t count, const float ambient[3],
                          const float* d_offsets, const int* d_ids, size_t row_begin, size_t row_count,
                          float* d_rgba, unsigned char* d_classes, void* stream) {
    return LightAsync(view, lights, count, ambient, nullptr, d_offsets, d_ids, row_begin, row_count, d_rgba, d_classes,
                      stream);
}

RTD_API int rtdLightHost(const char* scene_path, size_t width, size_t height, const rtd_light_host* lights, size_t count,
                         const float ambient[3], const float* offsets, const int* ids, size_t row_begin, size_t row_count,
                         float* rgba, unsigned char* classes) {
    return LightHost(scene_path, width, height, lights, count, ambient, nullptr, nullptr, offsets, ids, row_begin,
                     row_count, rgba, classes);
}

// Dynamic scenes (include/srt_motion.h): the rtm family. Checks in the order flags, camera / origin,
// handle, device buffer, so every refusal but the last is reachable without a device.
static_assert(RTM_REORDER == 0 && RTM_KEEP_ORDER == 1, "include/srt_motion.h flags");

namespace {

bool CheckedReorder(int flags) {
    if ((flags & ~RTM_KEEP_ORDER) != 0) {
        throw std::runtime_error("Unknown motion flags " + std::to_string(flags));
    }
    return (flags & RTM_KEEP_ORDER) == 0;
}

srt::Camera CheckedCameraArg(const float camera10[10]) {
    if (camera10 == nullptr) {
        throw std::runtime_error("Bad argument: camera10 is NULL");
    }
    return CheckedCamera(camera10);
}

}  // namespace

RTM_API int rtmSetCameraAsync(srt_device_scene scene, const float camera10[10], int flags, void* stream) {
    return Guarded([&] {
        const bool reorder = CheckedReorder(flags);
        const srt::Camera camera = CheckedCameraArg(camera10);
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->SetCamera(camera, reorder, static_cast<hipStream_t>(stream));
    });
}

RTM_API int rtmSetVerticesAsync(srt_device_scene scene, const float* d_vertices, int flags, void* stream) {
    return Guarded([&] {
        const bool reorder = CheckedReorder(flags);
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        srt::DeviceScene* s = FromHandle(scene);
        if (d_vertices == nullptr && s->triangles() != 0) {
            throw std::runtime_error("Bad buffer argument: d_vertices is NULL");
        }
        Bind bind(s->device());
        s->SetVertices(d_vertices, reorder, static_cast<hipStream_t>(stream));
    });
}

RTM_API int rtmGetCamera(srt_device_scene scene, float camera10[10]) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        if (camera10 == nullptr) {
            throw std::runtime_error("Bad argument: camera10 is NULL");
        }
        const srt::Camera& c = FromHandle(scene)->camera();
        std::copy(c.eye, c.eye + 3, camera10);
        std::copy(c.lookat, c.lookat + 3, camera10 + 3);
        std::copy(c.up, c.up + 3, camera10 + 6);
        camera10[9] = c.vfov_deg;
    });
}

RTM_API int rtmLightSetOriginAsync(rto_light light, const float origin3[3], int flags, void* stream) {
    return Guarded([&] {
        const bool reorder = CheckedReorder(flags);
        CheckedOrigin(origin3);
        srt::Camera cameras[srt::kOmniFaces];
        for (int k = 0; k < srt::kOmniFaces; ++k) {  // (all six before the first face moves)
            float c10[10];
            srt::OmniFaceCamera(origin3, k, c10);
            cameras[k] = CheckedCamera(c10);
        }
        if (light == nullptr) {
            throw std::runtime_error("Bad light handle");
        }
        Bind bind(light->device);
        for (int k = 0; k < srt::kOmniFaces; ++k) {
            light->faces[k]->SetCamera(cameras[k], reorder, static_cast<hipStream_t>(stream));
        }
    });
}

RTM_API int rtmLightSetVerticesAsync(rto_light light, const float* d_vertices, int flags, void* stream) {
    return Guarded([&] {
        const bool reorder = CheckedReorder(flags);
        if (light == nullptr) {
            throw std::runtime_error("Bad light handle");
        }
        if (d_vertices == nullptr && light->faces[0]->triangles() != 0) {
            throw std::runtime_error("Bad buffer argument: d_vertices is NULL");
        }
        Bind bind(light->device);
        for (auto& f : light->faces) {
            f->SetVertices(d_vertices, reorder, static_cast<hipStream_t>(stream));
        }
    });
}

RTM_API int rtmOrderHost(const float* vertices, unsigned long long n, const float camera10[10], unsigned* order,
                         float* normals) {
    return Guarded([&] {
        const srt::Camera camera = CheckedCameraArg(camera10);
        if (vertices == nullptr && n != 0) {
            throw std::runtime_error("Bad argument: vertices is NULL");
        }
        srt::OrderHost(vertices, n, camera, order, normals);
    });
}

// Vertex attributes (include/srt_surface.h): the rtv family.
static_assert(RTV_WRAP_CLAMP == srt::kSurfaceWrapClamp && RTV_FILTER_NEAREST == srt::kSurfaceFilterNearest &&
                  RTV_MODULATE == srt::kSurfaceModulate && RTV_MAX_TEXTURE == srt::kSurfaceMaxTexture &&
                  RTV_MAX_CHANNELS == srt::kSurfaceMaxChannels,
              "include/srt_surface.h constants");

namespace {

rtv_surface CheckedSurface(const rtv_surface* s) {
    if (s == nullptr) {
        throw std::runtime_error("Bad argument: surface is NULL");
    }
    if (s->struct_size != sizeof(rtv_surface)) {
        throw std::runtime_error("rtv_surface.struct_size is " + std::to_string(s->struct_size) + ", expected " +
                                 std::to_string(sizeof(rtv_surface)));
    }
    if ((s->flags & ~srt::kSurfaceFlags) != 0u) {
        throw std::runtime_error("rtv_surface.flags is " + std::to_string(s->flags) +
                                 ": only RTV_WRAP_CLAMP, RTV_FILTER_NEAREST and RTV_MODULATE are known");
    }
    if (s->texture != nullptr) {
        if (s->uvs == nullptr) {
            throw std::runtime_error("rtv_surface.texture is set but rtv_surface.uvs is NULL: a texture needs uvs");
        }
        if (s->tex_width < 1 || s->tex_width > RTV_MAX_TEXTURE) {
            throw std::runtime_error("rtv_surface.tex_width must be 1 to " + std::to_string(RTV_MAX_TEXTURE) + ", got " +
                                     std::to_string(s->tex_width));
        }
        if (s->tex_height < 1 || s->tex_height > RTV_MAX_TEXTURE) {
            throw std::runtime_error("rtv_surface.tex_height must be 1 to " + std::to_string(RTV_MAX_TEXTURE) +
                                     ", got " + std::to_string(s->tex_height));
        }
    }
    return *s;
}

rtv_outputs CheckedSurfaceOutputs(const rtv_outputs* o) {
    if (o == nullptr) {
        throw std::runtime_error("Bad argument: outputs is NULL");
    }
    if (o->struct_size != sizeof(rtv_outputs)) {
        throw std::runtime_error("rtv_outputs.struct_size is " + std::to_string(o->struct_size) + ", expected " +
                                 std::to_string(sizeof(rtv_outputs)));
    }
    return *o;
}

bool NoSurfacePlane(const rtv_outputs& o) {
    return o.normal == nullptr && o.albedo == nullptr && o.rgba == nullptr && o.uv == nullptr;
}

void CheckChannels(size_t channels) {
    if (channels < 1 || channels > RTV_MAX_CHANNELS) {
        throw std::runtime_error("Bad argument: channels must be 1 to " + std::to_string(RTV_MAX_CHANNELS) + ", got " +
                                 std::to_string(channels));
    }
}

void NotNull(const void* p, const char* name) {
    if (p == nullptr) {
        throw std::runtime_error(std::string("Bad buffer argument: ") + name + " is NULL");
    }
}

srt::SurfaceArgs SurfacePlanes(const rtv_surface& s, const rtv_outputs& o) {
    srt::SurfaceArgs a{};
    a.normals = s.normals;
    a.uvs = s.uvs;
    a.texture = s.texture;
    a.tex_width = s.tex_width;
    a.tex_height = s.tex_height;
    a.flags = s.flags;
    a.normal = o.normal;
    a.albedo = o.albedo;
    a.rgba = o.rgba;
    a.uv = o.uv;
    return a;
}

void SurfaceAsync(srt_device_scene scene, bool points, const float* d_where, const char* where_name, const int* d_ids,
                  size_t row_begin, size_t count, const rtv_surface* surface, const rtv_outputs* outputs, void* stream) {
    if (scene == nullptr) {
        throw std::runtime_error("Bad scene handle");
    }
    const rtv_surface s = CheckedSurface(surface);
    const rtv_outputs o = CheckedSurfaceOutputs(outputs);
    if (count != 0 && !NoSurfacePlane(o)) {
        NotNull(d_where, where_name);
        NotNull(d_ids, "d_ids");
    }
    srt::DeviceScene* d = FromHandle(scene);
    Bind bind(d->device());
    d->Surface(points, d_where, d_ids, row_begin, count, SurfacePlanes(s, o), static_cast<hipStream_t>(stream));
}

void InterpolateAsync(srt_device_scene scene, bool points, const float* d_where, const char* where_name,
                      const int* d_ids, size_t row_begin, size_t count, const float* d_table, size_t channels,
                      float* d_out, void* stream) {
    if (scene == nullptr) {
        throw std::runtime_error("Bad scene handle");
    }
    CheckChannels(channels);
    srt::DeviceScene* d = FromHandle(scene);
    if (count != 0) {
        NotNull(d_where, where_name);
        NotNull(d_ids, "d_ids");
        NotNull(d_out, "d_out");
        if (d->triangles() != 0) {
            NotNull(d_table, "d_table");
        }
    }
    Bind bind(d->device());
    d->Interpolate(points, d_where, d_ids, row_begin, count, d_table, channels, d_out, static_cast<hipStream_t>(stream));
}

}  // namespace

RTV_API int rtvSurfaceFrameAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids, size_t row_begin,
                                 size_t row_count, const rtv_surface* surface, const rtv_outputs* outputs,
                                 void* stream) {
    return Guarded(
        [&] { SurfaceAsync(scene, false, d_offsets, "d_offsets", d_ids, row_begin, row_count, surface, outputs, stream); });
}

RTV_API int rtvSurfacePointsAsync(srt_device_scene scene, const float* d_positions, const int* d_ids, size_t count,
                                  const rtv_surface* surface, const rtv_outputs* outputs, void* stream) {
    return Guarded([&] { SurfaceAsync(scene, true, d_positions, "d_positions", d_ids, 0, count, surface, outputs, stream); });
}

RTV_API int rtvInterpolateFrameAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids,
                                     size_t row_begin, size_t row_count, const float* d_table, size_t channels,
                                     float* d_out, void* stream) {
    return Guarded([&] {
        InterpolateAsync(scene, false, d_offsets, "d_offsets", d_ids, row_begin, row_count, d_table, channels, d_out,
                         stream);
    });
}

RTV_API int rtvInterpolatePointsAsync(srt_device_scene scene, const float* d_positions, const int* d_ids, size_t count,
                                      const float* d_table, size_t channels, float* d_out, void* stream) {
    return Guarded([&] {
        InterpolateAsync(scene, true, d_positions, "d_positions", d_ids, 0, count, d_table, channels, d_out, stream);
    });
}

RTV_API int rtvSurfaceHost(const char* scene_path, size_t width, size_t height, const float* positions, const int* ids,
                           size_t count, const rtv_surface* surface, const rtv_outputs* outputs) {
    return Guarded([&] {
        const rtv_surface s = CheckedSurface(surface);
        const rtv_outputs o = CheckedSurfaceOutputs(outputs);
        if (scene_path == nullptr || width == 0 || height == 0) {
            throw std::runtime_error("Bad argument");
        }
        if (count != 0 && !NoSurfacePlane(o)) {
            NotNull(positions, "positions");
            NotNull(ids, "ids");
        }
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostSurface(scene, width, height, positions, ids, count, s.normals, s.uvs, s.texture, s.tex_width,
                         s.tex_height, s.flags, o.normal, o.albedo, o.rgba, o.uv);
    });
}

RTV_API int rtvInterpolateHost(const char* scene_path, size_t width, size_t height, const float* positions,
                               const int* ids, size_t count, const float* table, size_t channels, float* out) {
    return Guarded([&] {
        CheckChannels(channels);
        if (scene_path == nullptr || width == 0 || height == 0) {
            throw std::runtime_error("Bad argument");
        }
        const srt::Scene scene = srt::LoadScene(scene_path);
        if (count != 0) {
            NotNull(positions, "positions");
            NotNull(ids, "ids");
            NotNull(out, "out");
            if (scene.triangle_count() != 0) {
                NotNull(table, "table");
            }
        }
        srt::HostInterpolate(scene, width, height, positions, ids, count, table, channels, out);
    });
}

RTV_API int rtvObjAttributesHost(const char* path, float* normals, float* uvs, int have[2]) {
    return Guarded([&] {
        if (path == nullptr) {
            throw std::runtime_error("Bad argument: path is NULL");
        }
        std::vector<float> n, t;
        bool any[2];
        srt::LoadObjAttributes(path, n, t, any);
        if (normals != nullptr) {
            std::copy(n.begin(), n.end(), normals);
        }
        if (uvs != nullptr) {
            std::copy(t.begin(), t.end(), uvs);
        }
        if (have != nullptr) {
            have[0] = any[0] ? 1 : 0;
            have[1] = any[1] ? 1 : 0;
        }
    });
}

// Lit surfaces (include/srt_material.h): the rtp family -- the rtd calls on an rtv surface. The
// surface and the material are checked here, before the lights; the rest is LightAsync / LightHost.
static_assert(RTP_MAX_SHININESS_LOG2 == srt::kMaterialMaxShininessLog2, "include/srt_material.h and material_math.h agree");

namespace {

// The surface (NULL: none) and the material (NULL: none) of an rtp call, as render.h's LitSurface.
srt::LitSurface CheckedLitSurface(const rtv_surface* surface, const rtp_material* material) {
    srt::LitSurface out{};
    if (surface != nullptr) {
        const rtv_surface s = CheckedSurface(surface);
        out.normals = s.normals;
        out.uvs = s.uvs;
        out.texture = s.texture;
        out.tex_width = s.tex_width;
        out.tex_height = s.tex_height;
        out.flags = s.flags;
    }
    if (material != nullptr) {
        if (material->struct_size != sizeof(rtp_material)) {
            throw std::runtime_error("rtp_material.struct_size is " + std::to_string(material->struct_size) +
                                     ", expected " + std::to_string(sizeof(rtp_material)));
        }
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(material->specular[k])) {
                throw std::runtime_error("rtp_material.specular value " + std::to_string(k) + " is not finite");
            }
            out.specular[k] = material->specular[k];
        }
        if (material->shininess_log2 < 0 || material->shininess_log2 > RTP_MAX_SHININESS_LOG2) {
            throw std::runtime_error("rtp_material.shininess_log2 must be 0 to " + std::to_string(RTP_MAX_SHININESS_LOG2) +
                                     ", got " + std::to_string(material->shininess_log2));
        }
        out.material = true;
        out.shininess_log2 = material->shininess_log2;
    }
    return out;
}

}  // namespace

RTP_API int rtpLightSurfaceAsync(srt_device_scene view, const rtd_light* lights, size_t count, const float ambient[3],
                                 const rtv_surface* surface, const rtp_material* material, const float* d_offsets,
                                 const int* d_ids, size_t row_begin, size_t row_count, float* d_rgba,
                                 unsigned char* d_classes, void* stream) {
    srt::LitSurface lit{};
    if (Guarded([&] { lit = CheckedLitSurface(surface, material); }) != 0) {
        return -1;
    }
    return LightAsync(view, lights, count, ambient, &lit, d_offsets, d_ids, row_begin, row_count, d_rgba, d_classes,
                      stream);
}

RTP_API int rtpLightSurfaceHost(const char* scene_path, size_t width, size_t height, const rtd_light_host* lights,
                                size_t count, const float ambient[3], const rtv_surface* surface,
                                const rtp_material* material, const float* offsets, const int* ids, size_t row_begin,
                                size_t row_count, float* rgba, unsigned char* classes) {
    srt::LitSurface lit{};
    if (Guarded([&] { lit = CheckedLitSurface(surface, material); }) != 0) {
        return -1;
    }
    const srt::HostSurfaceTables tables{lit.normals, lit.uvs, lit.texture, lit.tex_width, lit.tex_height, lit.flags};
    const srt::HostMaterial mat{{lit.specular[0], lit.specular[1], lit.specular[2]}, lit.shininess_log2};
    return LightHost(scene_path, width, height, lights, count, ambient, &tables, lit.material ? &mat : nullptr, offsets,
                     ids, row_begin, row_count, rgba, classes);
}

// Ray queries (include/srt_rays.h): the rtr family.
static_assert(RTR_RAY_FLOATS * sizeof(float) == sizeof(srt::Ray), "include/srt_rays.h and ray_math.h agree");

namespace {

void CheckRays(const float* rays, const char* name, bool device) {
    if (rays == nullptr) {
        throw std::runtime_error(std::string("Bad buffer argument: ") + name + " is NULL");
    }
    if (device && reinterpret_cast<std::uintptr_t>(rays) % 16 != 0) {
        throw std::runtime_error(std::string("Bad buffer argument: ") + name + " is not 16-byte aligned");
    }
}

bool CheckedBoxClause(int flags) {
    if ((flags & ~RTR_NO_BOX_CLAUSE) != 0) {
        throw std::runtime_error("Unknown ray flags " + std::to_string(flags));
    }
    return (flags & RTR_NO_BOX_CLAUSE) == 0;
}

}  // namespace

RTR_API int rtrBuildAsync(srt_device_scene scene, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->BuildRays(static_cast<hipStream_t>(stream));
    });
}

RTR_API int rtrClosestAsync(srt_device_scene scene, const float* d_rays, size_t count, int* d_ids, float* d_t,
                            float* d_bary, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        if (count != 0) {
            CheckRays(d_rays, "d_rays", true);
            if (d_ids == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_ids is NULL");
            }
            if (d_t == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_t is NULL");
            }
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Closest(d_rays, count, d_ids, d_t, d_bary, static_cast<hipStream_t>(stream));
    });
}

RTR_API int rtrOccludedAsync(srt_device_scene scene, const float* d_rays, size_t count, unsigned char* d_out,
                             void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        if (count != 0) {
            CheckRays(d_rays, "d_rays", true);
            if (d_out == nullptr) {
                throw std::runtime_error("Bad buffer argument: d_out is NULL");
            }
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Occluded(d_rays, count, d_out, static_cast<hipStream_t>(stream));
    });
}

RTR_API int rtrClosestHostFlags(const char* scene_path, const float* rays, size_t count, int* ids, float* t,
                                float* bary, int flags) {
    return Guarded([&] {
        const bool box_clause = CheckedBoxClause(flags);
        if (scene_path == nullptr) {
            throw std::runtime_error("Bad argument: scene_path is NULL");
        }
        if (count != 0) {
            CheckRays(rays, "rays", false);
            if (ids == nullptr) {
                throw std::runtime_error("Bad buffer argument: ids is NULL");
            }
            if (t == nullptr) {
                throw std::runtime_error("Bad buffer argument: t is NULL");
            }
        }
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostRayClosest(scene, rays, count, ids, t, bary, box_clause);
    });
}

RTR_API int rtrOccludedHostFlags(const char* scene_path, const float* rays, size_t count, unsigned char* out,
                                 int flags) {
    return Guarded([&] {
        const bool box_clause = CheckedBoxClause(flags);
        if (scene_path == nullptr) {
            throw std::runtime_error("Bad argument: scene_path is NULL");
        }
        if (count != 0) {
            CheckRays(rays, "rays", false);
            if (out == nullptr) {
                throw std::runtime_error("Bad buffer argument: out is NULL");
            }
        }
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostRayOccluded(scene, rays, count, out, box_clause);
    });
}

RTR_API int rtrClosestHost(const char* scene_path, const float* rays, size_t count, int* ids, float* t, float* bary) {
    return rtrClosestHostFlags(scene_path, rays, count, ids, t, bary, RTR_BOX_CLAUSE);
}

RTR_API int rtrOccludedHost(const char* scene_path, const float* rays, size_t count, unsigned char* out) {
    return rtrOccludedHostFlags(scene_path, rays, count, out, RTR_BOX_CLAUSE);
}

// Sampled visibility (include/srt_visibility.h): the rta family.
static_assert(RTA_HEMISPHERE == srt::kVisibilityHemisphere && RTA_AREA == srt::kVisibilityArea &&
                  RTA_MIRROR == srt::kVisibilityMirror && RTA_MAX_SAMPLES == srt::kVisibilityMaxSamples &&
                  RTA_ROTATIONS == srt::kVisibilityRotations,
              "include/srt_visibility.h and visibility_math.h agree");

namespace {

// The generator of a call, every field checked. visibility: a call that counts (no mirror).
srt::VisibilityGen CheckedGenerator(const rta_generator* g, bool visibility) {
    if (g == nullptr) {
        throw std::runtime_error("Bad argument: gen is NULL");
    }
    if (g->struct_size != sizeof(rta_generator)) {
        throw std::runtime_error("rta_generator.struct_size is " + std::to_string(g->struct_size) + ", expected " +
                                 std::to_string(sizeof(rta_generator)));
    }
    if (g->kind != RTA_HEMISPHERE && g->kind != RTA_AREA && g->kind != RTA_MIRROR) {
        throw std::runtime_error("rta_generator.kind is " + std::to_string(g->kind) +
                                 ", expected RTA_HEMISPHERE, RTA_AREA or RTA_MIRROR");
    }
    if (g->kind == RTA_MIRROR && visibility) {
        throw std::runtime_error("rta_generator.kind is RTA_MIRROR: the mirror generator is export only");
    }
    if (g->samples < 1 || g->samples > RTA_MAX_SAMPLES) {
        throw std::runtime_error("rta_generator.samples must be 1 to " + std::to_string(RTA_MAX_SAMPLES) + ", got " +
                                 std::to_string(g->samples));
    }
    if (g->kind == RTA_MIRROR && g->samples != 1) {
        throw std::runtime_error("rta_generator.samples must be 1 for RTA_MIRROR, got " + std::to_string(g->samples));
    }
    if (g->kind != RTA_MIRROR && g->d_samples == nullptr) {
        throw std::runtime_error("rta_generator.d_samples is NULL");
    }
    srt::VisibilityGen out{};
    out.kind = g->kind;
    out.count = g->samples;
    out.samples = g->d_samples;
    out.rotations = g->kind == RTA_HEMISPHERE ? g->d_rotations : nullptr;
    if (g->kind == RTA_AREA) {
        const struct {
            const char* name;
            const float* v;
        } fields[3] = {{"corner", g->corner}, {"eu", g->eu}, {"ev", g->ev}};
        for (const auto& f : fields) {
            for (int k = 0; k < 3; ++k) {
                if (!std::isfinite(f.v[k])) {
                    throw std::runtime_error(std::string("rta_generator.") + f.name + " is not finite");
                }
            }
        }
        std::memcpy(out.corner, g->corner, sizeof out.corner);
        std::memcpy(out.eu, g->eu, sizeof out.eu);
        std::memcpy(out.ev, g->ev, sizeof out.ev);
    }
    out.tmin = g->tmin;
    out.tmax = g->tmax;
    return out;
}

rta_outputs CheckedVisibilityOutputs(const rta_outputs* o) {
    if (o == nullptr) {
        throw std::runtime_error("Bad argument: outputs is NULL");
    }
    if (o->struct_size != sizeof(rta_outputs)) {
        throw std::runtime_error("rta_outputs.struct_size is " + std::to_string(o->struct_size) + ", expected " +
                                 std::to_string(sizeof(rta_outputs)));
    }
    return *o;
}

void CheckElements(const float* where, const char* where_name, const int* ids, const char* ids_name) {
    if (where == nullptr) {
        throw std::runtime_error(std::string("Bad buffer argument: ") + where_name + " is NULL");
    }
    if (ids == nullptr) {
        throw std::runtime_error(std::string("Bad buffer argument: ") + ids_name + " is NULL");
    }
}

int VisibilityAsync(srt_device_scene scene, bool points, const float* d_where, const char* where_name,
                    const int* d_ids, size_t row_begin, size_t count, const rta_generator* gen,
                    const rta_outputs* outputs, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        const srt::VisibilityGen g = CheckedGenerator(gen, true);
        const rta_outputs o = CheckedVisibilityOutputs(outputs);
        if (count != 0 && (o.visible != nullptr || o.fraction != nullptr)) {
            CheckElements(d_where, where_name, d_ids, "d_ids");
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Visibility(points, d_where, d_ids, row_begin, count, g, o.visible, o.fraction,
                      static_cast<hipStream_t>(stream));
    });
}

int VisibilityRaysAsync(srt_device_scene scene, bool points, const float* d_where, const char* where_name,
                        const int* d_ids, size_t row_begin, size_t count, const rta_generator* gen, float* d_rays,
                        void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        const srt::VisibilityGen g = CheckedGenerator(gen, false);
        if (count != 0) {
            CheckElements(d_where, where_name, d_ids, "d_ids");
            CheckRays(d_rays, "d_rays", true);
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->VisibilityRays(points, d_where, d_ids, row_begin, count, g, d_rays, static_cast<hipStream_t>(stream));
    });
}

}  // namespace

RTA_API int rtaVisibilityFrameAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids, size_t row_begin,
                                    size_t row_count, const rta_generator* gen, const rta_outputs* outputs,
                                    void* stream) {
    return VisibilityAsync(scene, false, d_offsets, "d_offsets", d_ids, row_begin, row_count, gen, outputs, stream);
}

RTA_API int rtaVisibilityPointsAsync(srt_device_scene scene, const float* d_positions, const int* d_ids, size_t count,
                                     const rta_generator* gen, const rta_outputs* outputs, void* stream) {
    return VisibilityAsync(scene, true, d_positions, "d_positions", d_ids, 0, count, gen, outputs, stream);
}

RTA_API int rtaRaysFrameAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids, size_t row_begin,
                              size_t row_count, const rta_generator* gen, float* d_rays, void* stream) {
    return VisibilityRaysAsync(scene, false, d_offsets, "d_offsets", d_ids, row_begin, row_count, gen, d_rays, stream);
}

RTA_API int rtaRaysPointsAsync(srt_device_scene scene, const float* d_positions, const int* d_ids, size_t count,
                               const rta_generator* gen, float* d_rays, void* stream) {
    return VisibilityRaysAsync(scene, true, d_positions, "d_positions", d_ids, 0, count, gen, d_rays, stream);
}

RTA_API int rtaVisibilityHost(const char* scene_path, size_t width, size_t height, const float* positions,
                              const int* ids, size_t count, const rta_generator* gen, const rta_outputs* outputs) {
    return Guarded([&] {
        const srt::VisibilityGen g = CheckedGenerator(gen, true);
        const rta_outputs o = CheckedVisibilityOutputs(outputs);
        if (scene_path == nullptr) {
            throw std::runtime_error("Bad argument: scene_path is NULL");
        }
        if (width == 0 || height == 0) {
            throw std::runtime_error("Bad argument: frame dimensions must be non-zero");
        }
        if (count == 0 || (o.visible == nullptr && o.fraction == nullptr)) {
            return;
        }
        CheckElements(positions, "positions", ids, "ids");
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostVisibility(scene, width, height, positions, ids, count, g, o.visible, o.fraction);
    });
}

RTA_API int rtaRaysHost(const char* scene_path, size_t width, size_t height, const float* positions, const int* ids,
                        size_t count, const rta_generator* gen, float* rays) {
    return Guarded([&] {
        const srt::VisibilityGen g = CheckedGenerator(gen, false);
        if (scene_path == nullptr) {
            throw std::runtime_error("Bad argument: scene_path is NULL");
        }
        if (width == 0 || height == 0) {
            throw std::runtime_error("Bad argument: frame dimensions must be non-zero");
        }
        if (count == 0) {
            return;
        }
        CheckElements(positions, "positions", ids, "ids");
        CheckRays(rays, "rays", false);
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostVisibilityRays(scene, width, height, positions, ids, count, g, rays);
    });
}

#ifdef SRT_DIAG
// Diagnostic build only (make diag): not part of include/srt_render.h.
ML_API_ENTRY int srtDiagRead(void* host, size_t bytes) {
    return Guarded([&] { srt::HipCheck(srt::DiagRead(host, bytes), "srtDiagRead"); });
}
#endif

}  // extern "C"

// Lit ray hits (include/srt_hits.h): the rth family. The lights are the rtd family's, collected and
// checked by the same code, so a refused light is refused in the same words.
namespace {

// The blend of a call: its base (null without a blend) and weight, the struct checked.
const float* CheckedBlend(const rth_blend* blend, bool device, float weight[3]) {
    weight[0] = weight[1] = weight[2] = 0.f;
    if (blend == nullptr) {
        return nullptr;
    }
    if (blend->struct_size != sizeof(rth_blend)) {
        throw std::runtime_error("Light hits: rth_blend.struct_size is " + std::to_string(blend->struct_size) +
                                 ", expected " + std::to_string(sizeof(rth_blend)));
    }
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(blend->weight[k])) {
            throw std::runtime_error("Light hits: weight value " + std::to_string(k) + " is not finite");
        }
        weight[k] = blend->weight[k];
    }
    return blend->d_base;
}

void CheckHitBuffers(const float* rays, const int* ids, const float* t, size_t elements, const rth_blend* blend,
                     const float* base, const float* rgba, bool device) {
    if (elements > 0x7FFFFFFFull) {
        throw std::runtime_error("Light hits: at most 2147483647 elements per call, got " + std::to_string(elements));
    }
    if (elements == 0) {
        return;
    }
    const std::string d = device ? "d_" : "";
    CheckRays(rays, (d + "rays").c_str(), device);
    if (ids == nullptr) {
        throw std::runtime_error("Bad buffer argument: " + d + "ids is NULL");
    }
    if (t == nullptr) {
        throw std::runtime_error("Bad buffer argument: " + d + "t is NULL");
    }
    if (blend != nullptr) {
        CheckRays(base, "blend->d_base", device);
    }
    CheckRays(rgba, (d + "rgba").c_str(), device);
}

}  // namespace

RTH_API int rthLightHitsAsync(srt_device_scene scene, const rtd_light* lights, size_t count, const float ambient[3],
                              const float* d_rays, const int* d_ids, const float* d_t, size_t elements,
                              const rth_blend* blend, float* d_rgba, unsigned char* d_classes, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle: scene is NULL");
        }
        srt::DeviceScene::CheckLightCount(count);
        if (count != 0 && lights == nullptr) {
            throw std::runtime_error("Bad argument: lights is NULL");
        }
        if (ambient == nullptr) {
            throw std::runtime_error("Bad argument: ambient is NULL");
        }
        std::vector<srt::DeviceScene::Light> in(count);
        std::vector<const srt::DeviceScene*> scenes(count * srt::kOmniFaces);
        CollectDeviceLights(lights, count, in.data(), scenes.data());
        float weight[3];
        const float* d_base = CheckedBlend(blend, true, weight);
        CheckHitBuffers(d_rays, d_ids, d_t, elements, blend, d_base, d_rgba, true);
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->LightHits(in.data(), count, ambient, d_rays, d_ids, d_t, elements, d_base, weight, d_rgba, d_classes,
                     static_cast<hipStream_t>(stream));
    });
}

RTH_API int rthLightHitsHost(const char* scene_path, const rtd_light_host* lights, size_t count, const float ambient[3],
                             const float* rays, const int* ids, const float* t, size_t elements,
                             const rth_blend* blend, float* rgba, unsigned char* classes) {
    return Guarded([&] {
        if (scene_path == nullptr) {
            throw std::runtime_error("Bad argument: scene_path is NULL");
        }
        srt::DeviceScene::CheckLightCount(count);
        if (count != 0 && lights == nullptr) {
            throw std::runtime_error("Bad argument: lights is NULL");
        }
        if (ambient == nullptr) {
            throw std::runtime_error("Bad argument: ambient is NULL");
        }
        std::vector<srt::HostLight> in;
        CollectHostLights(lights, count, ambient, in);
        float weight[3];
        const float* base = CheckedBlend(blend, false, weight);
        CheckHitBuffers(rays, ids, t, elements, blend, base, rgba, false);
        if (elements == 0) {
            return;
        }
        const srt::Scene scene = srt::LoadScene(scene_path);
        srt::HostLightHits(scene, in.data(), count, ambient, rays, ids, t, elements, base, weight, rgba, classes);
    });
}

// Sampled radiance (include/srt_radiance.h): the rti family. The generator is the rta family's, the
// lights the rtd family's and the blend the rth family's, each checked by that family's code.
namespace {

struct RadianceOptions {
    bool modulate;
    const float* base;  // null without a blend
    float weight[3];
};

RadianceOptions CheckedRadianceOptions(const rti_options* options) {
    RadianceOptions out{false, nullptr, {0.f, 0.f, 0.f}};
    if (options == nullptr) {
        return out;
    }
    if (options->struct_size != sizeof(rti_options)) {
        throw std::runtime_error("Radiance: rti_options.struct_size is " + std::to_string(options->struct_size) +
                                 ", expected " + std::to_string(sizeof(rti_options)));
    }
    out.modulate = options->modulate != 0;
    const rth_blend* blend = options->blend;
    if (blend == nullptr) {
        return out;
    }
    if (blend->struct_size != sizeof(rth_blend)) {
        throw std::runtime_error("Radiance: rth_blend.struct_size is " + std::to_string(blend->struct_size) +
                                 ", expected " + std::to_string(sizeof(rth_blend)));
    }
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(blend->weight[k])) {
            throw std::runtime_error("Radiance: blend weight value " + std::to_string(k) + " is not finite");
        }
        out.weight[k] = blend->weight[k];
    }
    if (blend->d_base == nullptr) {
        throw std::runtime_error("Bad buffer argument: blend->d_base is NULL");
    }
    out.base = blend->d_base;
    return out;
}

// The generator of a radiance call: rta's checks, then the kinds whose rays aim at surfaces.
srt::VisibilityGen CheckedRadianceGenerator(const rta_generator* gen) {
    const srt::VisibilityGen g = CheckedGenerator(gen, false);
    if (g.kind == RTA_AREA) {
        throw std::runtime_error(
            "rta_generator.kind is RTA_AREA: its rays aim at a light, not at surfaces; radiance takes RTA_HEMISPHERE or "
            "RTA_MIRROR");
    }
    return g;
}

void CheckRadianceBuffers(const float* where, const char* where_name, const int* ids, const char* ids_name,
                          const RadianceOptions& o, const float* rgba, const char* rgba_name, bool device) {
    CheckElements(where, where_name, ids, ids_name);
    if (o.base != nullptr) {
        CheckRays(o.base, "blend->d_base", device);
    }
    CheckRays(rgba, rgba_name, device);
}

int RadianceAsync(srt_device_scene scene, const rtd_light* lights, size_t count, const float ambient[3], bool points,
                  const float* d_where, const char* where_name, const int* d_ids, size_t row_begin, size_t elements,
                  const rta_generator* gen, const rti_options* options, float* d_rgba, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle: scene is NULL");
        }
        srt::DeviceScene::CheckLightCount(count);
        if (count != 0 && lights == nullptr) {
            throw std::runtime_error("Bad argument: lights is NULL");
        }
        if (ambient == nullptr) {
            throw std::runtime_error("Bad argument: ambient is NULL");
        }
        const srt::VisibilityGen g = CheckedRadianceGenerator(gen);
        const RadianceOptions o = CheckedRadianceOptions(options);
        std::vector<srt::DeviceScene::Light> in(count);
        std::vector<const srt::DeviceScene*> scenes(count * srt::kOmniFaces);
        CollectDeviceLights(lights, count, in.data(), scenes.data());
        if (elements != 0) {
            CheckRadianceBuffers(d_where, where_name, d_ids, "d_ids", o, d_rgba, "d_rgba", true);
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->Radiance(in.data(), count, ambient, points, d_where, d_ids, row_begin, elements, g, o.modulate, o.base,
                    o.weight, d_rgba, static_cast<hipStream_t>(stream));
    });
}

}  // namespace

extern "C" {

RTI_API int rtiRadianceFrameAsync(srt_device_scene scene, const rtd_light* lights, size_t count, const float ambient[3],
                                  const float* d_offsets, const int* d_ids, size_t row_begin, size_t row_count,
                                  const rta_generator* gen, const rti_options* options, float* d_rgba, void* stream) {
    return RadianceAsync(scene, lights, count, ambient, false, d_offsets, "d_offsets", d_ids, row_begin, row_count, gen,
                         options, d_rgba, stream);
}

RTI_API int rtiRadiancePointsAsync(srt_device_scene scene, const rtd_light* lights, size_t count, const float ambient[3],
                                   const float* d_positions, const int* d_ids, size_t elements,
                                   const rta_generator* gen, const rti_options* options, float* d_rgba, void* stream) {
    return RadianceAsync(scene, lights, count, ambient, true, d_positions, "d_positions", d_ids, 0, elements, gen,
                         options, d_rgba, stream);
}

RTI_API int rtiRadianceHost(const char* scene_path, size_t width, size_t height, const rtd_light_host* lights,
                            size_t count, const float ambient[3], const float* positions, const int* ids,
                            size_t elements, const rta_generator* gen, const rti_options* options, float* rgba) {
    return Guarded([&] {
        if (scene_path == nullptr) {
            throw std::runtime_error("Bad argument: scene_path is NULL");
        }
        if (width == 0 || height == 0) {
            throw std::runtime_error("Bad argument: frame dimensions must be non-zero");
        }
        srt::DeviceScene::CheckLightCount(count);
        if (count != 0 && lights == nullptr) {
            throw std::runtime_error("Bad argument: lights is NULL");
        }
        if (ambient == nullptr) {
            throw std::runtime_error("Bad argument: ambient is NULL");
        }
        const srt::VisibilityGen g = CheckedRadianceGenerator(gen);
        const RadianceOptions o = CheckedRadianceOptions(options);
        std::vector<srt::HostLight> in;
        CollectHostLights(lights, count, ambient, in);
        if (elements > 0x7FFFFFFFull) {
            throw std::runtime_error("Radiance: at most 2147483647 elements per call, got " + std::to_string(elements));
        }
        if (elements == 0) {
            return;
        }
        CheckRadianceBuffers(positions, "positions", ids, "ids", o, rgba, "rgba", false);
        const srt::Scene scene = srt::LoadScene(scene_path);
        const srt::RadianceStore store{o.modulate, o.base, {o.weight[0], o.weight[1], o.weight[2]}, rgba};
        srt::HostRadiance(scene, width, height, in.data(), count, ambient, positions, ids, elements, g, store);
    });
}

}  // extern "C"

// Pinned offsets (include/srt_pins.h): the rtn family.
static_assert(RTN_MAX_PINS == srt::PinTable::kMaxPins, "include/srt_pins.h RTN_MAX_PINS");

RTN_API int rtnPinOffsetsAsync(srt_device_scene scene, const float* d_offsets, void* stream) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        if (d_offsets == nullptr) {
            throw std::runtime_error("Bad buffer argument");
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->PinOffsets(d_offsets, static_cast<hipStream_t>(stream));
    });
}

RTN_API int rtnUnpinOffsets(srt_device_scene scene, const float* d_offsets) {
    return Guarded([&] {
        if (scene == nullptr) {
            throw std::runtime_error("Bad scene handle");
        }
        if (d_offsets == nullptr) {
            throw std::runtime_error("Bad buffer argument");
        }
        srt::DeviceScene* s = FromHandle(scene);
        Bind bind(s->device());
        s->UnpinOffsets(d_offsets);
    });
}
