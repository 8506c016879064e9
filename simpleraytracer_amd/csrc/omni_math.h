// The omni-light shadow test: a point light as six cube-face frames (render.hip OmniShadowKernel;
// DESIGN.md section 2 "Omni shadow"). Host and device share it (cpu_render.cpp HostOmniShadow, the
// host answer rtoShadowHost), so both make the same face choice from the same float expressions.
//
// Face k is the camera (eye = o, lookat = fl32(o + axis_k), up_k, vfov = kOmniVfovDeg) at F x F:
//   k  axis         up
//   0  (+1, 0, 0)   (0, 1, 0)
//   1  (-1, 0, 0)   (0, 1, 0)
//   2  (0, +1, 0)   (0, 0, -1)
//   3  (0, -1, 0)   (0, 0, +1)
//   4  (0, 0, +1)   (0, 1, 0)
//   5  (0, 0, -1)   (0, 1, 0)
// 92 degrees, not 90: a point whose major axis selects face k projects to |g - 1/2| <= 1/2 / tan 46
// = 0.4828 there, a guard of 0.0172 of the frame on every side, four orders of magnitude above the
// rounding of the projection, so shadow_math.h's frustum test never fires for the selected face.
//
// The face of q = P - o (shadow_math.h ShadowOffset): a_k = |q_k|; m = 0; if a_1 > a_m: m = 1;
// if a_2 > a_m: m = 2; face = 2 m + (q_m < 0 ? 1 : 0). Ties go to the lower axis, a NaN component
// never wins a comparison, q_m = +-0 picks the + face.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace srt {

constexpr int kOmniFaces = 6;
constexpr float kOmniVfovDeg = 92.f;
constexpr float kOmniOriginMax = 65536.f;  // |o_k| <= 2^16: fl32(o + axis) stays within the guard
constexpr unsigned char kOmniNoFace = 255;  // the face plane of a class-3 pixel

// axis[3], up[3] per face.
constexpr float kOmniFaceTable[kOmniFaces][6] = {
    {1.f, 0.f, 0.f, 0.f, 1.f, 0.f},  {-1.f, 0.f, 0.f, 0.f, 1.f, 0.f}, {0.f, 1.f, 0.f, 0.f, 0.f, -1.f},
    {0.f, -1.f, 0.f, 0.f, 0.f, 1.f}, {0.f, 0.f, 1.f, 0.f, 1.f, 0.f},  {0.f, 0.f, -1.f, 0.f, 1.f, 0.f},
};

// camera10 = eye, lookat, up, vfov_deg of face `face` (0 .. 5) of the light at `origin`.
inline void OmniFaceCamera(const float origin[3], int face, float camera10[10]) {
    for (int k = 0; k < 3; ++k) {
        camera10[k] = origin[k];
        camera10[3 + k] = origin[k] + kOmniFaceTable[face][k];
        camera10[6 + k] = kOmniFaceTable[face][3 + k];
    }
    camera10[9] = kOmniVfovDeg;
}

// Selects, not an indexed array: the kernel keeps q in registers.
__host__ __device__ inline int OmniFace(const float q[3]) {
    const float a0 = fabsf(q[0]), a1 = fabsf(q[1]), a2 = fabsf(q[2]);
    int m = 0;
    float am = a0, qm = q[0];
    if (a1 > am) {
        m = 1;
        am = a1;
        qm = q[1];
    }
    if (a2 > am) {
        m = 2;
        qm = q[2];
    }
    return 2 * m + (qm < 0.f ? 1 : 0);
}

}  // namespace srt
