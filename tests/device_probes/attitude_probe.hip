// Test probe (not product): the attitude helpers of pyflyt_amd/csrc/uav_device.hpp, one small kernel each, on a list of points.
// tests/test_gpu_attitude.py compiles this file with the product's compiler flags, calls attitude_probe() through ctypes and compares
// with tests/attitude_ref.py in float64. Each kernel loads, calls and stores, nothing else. Workgroups of 64: a wave is a workgroup,
// so the test decides which points share a wave.
#include <hip/hip_runtime.h>
#include "../../pyflyt_amd/csrc/uav_device.hpp"

namespace {
using namespace pf;

enum {
  P_ROT = 0,        // q[4]                 -> R[9] row major
  P_MUL,            // q[4] v[3]            -> R v [3], R^T v [3], R^T (R v) [3]
  P_EULER,          // q[4]                 -> rpy[3]                   euler_from_quat (libm)
  P_EULER_FAST,     // q[4]                 -> rpy[3]                   euler_from_quat_fast
  P_QUAT,           // rpy[3]               -> q[4]                     quat_from_euler
  P_CANON,          // q[4]                 -> q[4]                     canon_quat
  P_HALF,           // c s                  -> ch sh                    half_angle
  P_HALF_QUAT,      // cr sr cp sp cy sy    -> q[4]                     quat_from_half_angles
  P_ATAN2,          // y x                  -> r                        fast_atan2
  P_ATAN2_X2,       // y0 x0 y1 x1          -> r0 r1                    fast_atan2_x2, constants from atan2_consts()
  P_ASIN,           // x                    -> r                        fast_asin
  P_SINCOS_SMALL,   // x                    -> sin cos                  sincos_small
  P_SINCOS_TURNS,   // u                    -> sin cos                  sincos_turns
  P_SINCOS_ANGLE,   // a                    -> sin cos                  dogfight.hpp:129-132 (sincos_angle), restated below
  P_INTEGRATE,      // q[4] w[3] half_dt    -> q[4]                     quat_integrate
  P_COUNT
};
constexpr int in_floats(int w) {
  constexpr int t[P_COUNT] = {4, 7, 4, 4, 3, 4, 2, 6, 2, 4, 1, 1, 1, 1, 8};
  return t[w];
}
constexpr int out_floats(int w) {
  constexpr int t[P_COUNT] = {9, 9, 3, 3, 4, 4, 2, 4, 1, 2, 1, 2, 2, 2, 4};
  return t[w];
}

template <int W>
__global__ void probe_kernel(const float* in, float* out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float* x = in + (size_t)i * in_floats(W);
  float* o = out + (size_t)i * out_floats(W);
  if constexpr (W == P_ROT) {
    const m3 R = rot_from_quat(quat{x[0], x[1], x[2], x[3]});
    o[0] = R.m00; o[1] = R.m01; o[2] = R.m02; o[3] = R.m10; o[4] = R.m11; o[5] = R.m12; o[6] = R.m20; o[7] = R.m21; o[8] = R.m22;
  } else if constexpr (W == P_MUL) {
    const m3 R = rot_from_quat(quat{x[0], x[1], x[2], x[3]});
    const v3 v{x[4], x[5], x[6]};
    const v3 a = mul(R, v), b = mulT(R, v), c = mulT(R, a);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = b.x; o[4] = b.y; o[5] = b.z; o[6] = c.x; o[7] = c.y; o[8] = c.z;
  } else if constexpr (W == P_EULER) {
    const v3 e = euler_from_quat(quat{x[0], x[1], x[2], x[3]});
    o[0] = e.x; o[1] = e.y; o[2] = e.z;
  } else if constexpr (W == P_EULER_FAST) {
    const v3 e = euler_from_quat_fast(quat{x[0], x[1], x[2], x[3]});
    o[0] = e.x; o[1] = e.y; o[2] = e.z;
  } else if constexpr (W == P_QUAT) {
    const quat q = quat_from_euler(v3{x[0], x[1], x[2]});
    o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
  } else if constexpr (W == P_CANON) {
    const quat q = canon_quat(quat{x[0], x[1], x[2], x[3]});
    o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
  } else if constexpr (W == P_HALF) {
    float ch, sh;
    half_angle(x[0], x[1], ch, sh);
    o[0] = ch; o[1] = sh;
  } else if constexpr (W == P_HALF_QUAT) {
    const quat q = quat_from_half_angles(x[0], x[1], x[2], x[3], x[4], x[5]);
    o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
  } else if constexpr (W == P_ATAN2) {
    o[0] = fast_atan2(x[0], x[1]);
  } else if constexpr (W == P_ATAN2_X2) {
    const Atan2C k = atan2_consts();
    const f2 r = fast_atan2_x2(f2{x[0], x[2]}, f2{x[1], x[3]}, k);
    o[0] = r.x; o[1] = r.y;
  } else if constexpr (W == P_ASIN) {
    o[0] = fast_asin(x[0]);
  } else if constexpr (W == P_SINCOS_SMALL) {
    float s, c;
    sincos_small(x[0], s, c);
    o[0] = s; o[1] = c;
  } else if constexpr (W == P_SINCOS_TURNS) {
    float s, c;
    sincos_turns(x[0], s, c);
    o[0] = s; o[1] = c;
  } else if constexpr (W == P_SINCOS_ANGLE) {
    // dogfight.hpp cannot be included without its kernels (it pulls in the Fixedwing vehicle and the env step): sincos_angle,
    // dogfight.hpp:129-132, word for word
    float s, c;
    const float u = x[0] * (0.5f / kPi);
    sincos_turns(u - __builtin_floorf(u), s, c);
    o[0] = s; o[1] = c;
  } else {
    const quat q = quat_integrate(quat{x[0], x[1], x[2], x[3]}, v3{x[4], x[5], x[6]}, x[7]);
    o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
  }
}

template <int W>
void launch(int which, const float* din, float* dout, int n) {
  if constexpr (W < P_COUNT) {
    if (which == W) hipLaunchKernelGGL(probe_kernel<W>, dim3((n + 63) / 64), dim3(64), 0, 0, din, dout, n);
    else launch<W + 1>(which, din, dout, n);
  }
}
}  // namespace

// floats per point, in and out, of routine `which`; 1 for an unknown one
extern "C" int attitude_probe_strides(int which, int* in_stride, int* out_stride) {
  if (which < 0 || which >= P_COUNT) return 1;
  *in_stride = in_floats(which); *out_stride = out_floats(which);
  return 0;
}

// 0 = done; > 0: the hip call that failed; < 0: refused before any launch. n_in, n_out: the floats `in` and `out` hold.
extern "C" int attitude_probe(int which, const float* in, size_t n_in, float* out, size_t n_out, int n) {
  int is, os;
  if (attitude_probe_strides(which, &is, &os) != 0 || n <= 0 || !in || !out) return -1;
  if (n_in != (size_t)n * is || n_out != (size_t)n * os) return -2;
  float *din = nullptr, *dout = nullptr;
  const size_t ib = n_in * sizeof(float), ob = n_out * sizeof(float);
  int rc = 0;
  if (hipMalloc(&din, ib) != hipSuccess) rc = 1;
  if (!rc && hipMalloc(&dout, ob) != hipSuccess) rc = 2;
  if (!rc && hipMemcpy(din, in, ib, hipMemcpyHostToDevice) != hipSuccess) rc = 3;
  if (!rc && hipMemset(dout, 0xff, ob) != hipSuccess) rc = 4;  // (a point the kernel skipped reads back as NaN)
  if (!rc) {
    launch<0>(which, din, dout, n);
    if (hipGetLastError() != hipSuccess) rc = 5;
  }
  if (!rc && hipDeviceSynchronize() != hipSuccess) rc = 6;
  if (!rc && hipMemcpy(out, dout, ob, hipMemcpyDeviceToHost) != hipSuccess) rc = 7;
  const int frc = (hipFree(din) != hipSuccess) | (hipFree(dout) != hipSuccess);
  if (!rc && frc) rc = 8;
  return rc;
}
