// Test probe: the device math the kernels share (csrc/ta_math.h, ta_dual.h, ta_reduce.h), one primitive
// per launcher, so that tests/test_gpu_math.py can hold each of them to a high-precision reference.
// A shared object of its own (tests/math_probe.py builds it with the library's compile flags); the
// product library and its ABI do not know it.
//
// Layout of every launcher but mp_lane_sums: `in` holds NI rows of n doubles, `out` NO rows of n doubles
// (row-major; integer arguments travel as doubles, they are small). Every launcher returns TA_OK,
// TA_ERR_INVALID or TA_ERR_HIP.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "tensoralloy_amd.h"
#include "ta_device.h"
#include "ta_math.h"
#include "ta_dual.h"
#include "ta_reduce.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;

// out[k][i] = op(in[.][i])[k]: a bounds-checked grid-stride sweep
template <class Op>
__global__ __launch_bounds__(kThreads) void map_kernel(const double *in, double *out, int64_t n, Op op) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    double x[Op::NI], y[Op::NO];
#pragma unroll
    for (int k = 0; k < Op::NI; ++k) x[k] = in[(size_t)k * n + i];
    op(x, y);
#pragma unroll
    for (int k = 0; k < Op::NO; ++k) out[(size_t)k * n + i] = y[k];
  }
}

struct DeviceBuf {
  void *p = nullptr;
  ~DeviceBuf() {
    if (p) (void)hipFree(p);
  }
};

#define MP_CHECK(expr)                       \
  do {                                       \
    if ((expr) != hipSuccess) {              \
      (void)hipGetLastError();               \
      return TA_ERR_HIP;                     \
    }                                        \
  } while (0)

int grid_for(int64_t n) {
  const int64_t blocks = (n + kThreads - 1) / kThreads;
  return (int)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

template <class Op>
int run_map(const double *in, double *out, int64_t n, Op op) {
  if (!in || !out || n < 0) return TA_ERR_INVALID;
  if (n == 0) return TA_OK;
  DeviceBuf din, dout;
  const size_t bin = sizeof(double) * Op::NI * (size_t)n, bout = sizeof(double) * Op::NO * (size_t)n;
  MP_CHECK(hipMalloc(&din.p, bin));
  MP_CHECK(hipMalloc(&dout.p, bout));
  MP_CHECK(hipMemcpy(din.p, in, bin, hipMemcpyHostToDevice));
  MP_CHECK(hipMemset(dout.p, 0xff, bout));  // an element the kernel skips comes back as NaN
  hipLaunchKernelGGL(map_kernel<Op>, dim3(grid_for(n)), dim3(kThreads), 0, 0, (const double *)din.p,
                     (double *)dout.p, n, op);
  MP_CHECK(hipGetLastError());
  MP_CHECK(hipDeviceSynchronize());
  MP_CHECK(hipMemcpy(out, dout.p, bout, hipMemcpyDeviceToHost));
  return TA_OK;
}

struct ExpOp {
  static constexpr int NI = 1, NO = 1;
  __device__ void operator()(const double *x, double *y) const { y[0] = ta::ta_exp(x[0]); }
};

// f, df of cutoff_u; f, df, d2f of cutoff_u2; f of cutoff_u_value
struct CutoffOp {
  static constexpr int NI = 1, NO = 6;
  int kind;
  __device__ void operator()(const double *x, double *y) const {
    ta::cutoff_u(kind, x[0], y[0], y[1]);
    ta::cutoff_u2(kind, x[0], y[2], y[3], y[4]);
    y[5] = ta::cutoff_u_value(kind, x[0]);
  }
};

struct SoftplusOp {
  static constexpr int NI = 1, NO = 2;
  __device__ void operator()(const double *x, double *y) const { ta::softplus_fn(x[0], y[0], y[1]); }
};

struct RcpOp {
  static constexpr int NI = 1, NO = 1;
  __device__ void operator()(const double *x, double *y) const { y[0] = ta::rcp_1_3(x[0]); }
};

// h, dh of activation_fn; h, dh, d2h of activation_fn2
struct ActivationOp {
  static constexpr int NI = 1, NO = 5;
  int act;
  __device__ void operator()(const double *x, double *y) const {
    ta::activation_fn(act, x[0], y[0], y[1]);
    ta::activation_fn2(act, x[0], y[2], y[3], y[4]);
  }
};

// in: base, zi
struct PowIntOp {
  static constexpr int NI = 2, NO = 1;
  __device__ void operator()(const double *x, double *y) const { y[0] = ta::pow_int_m1(x[0], (int)x[1]); }
};

// in: x, exponent; out: safe_pow_value(x, exponent), safe_pow_grad(x, exponent)
struct SafePowOp {
  static constexpr int NI = 2, NO = 2;
  int safe;
  __device__ void operator()(const double *x, double *y) const {
    y[0] = ta::safe_pow_value(safe, x[0], x[1]);
    y[1] = ta::safe_pow_grad(safe, x[0], x[1]);
  }
};

// in: opcode, a.v, a.d, b.v, b.d; out: v, d. Opcodes 0-22: the Dual operators and t_* functions, where
// a "double" operand is the value of that Dual; opcode + 256: the same expression on plain doubles (d = 0).
struct DualOp {
  static constexpr int NI = 5, NO = 2;
  __device__ void operator()(const double *x, double *y) const {
    using ta::Dual;
    const int op = (int)x[0];
    const Dual a{x[1], x[2]}, b{x[3], x[4]};
    Dual r{__builtin_nan(""), __builtin_nan("")};
    double p = __builtin_nan("");
    switch (op) {
      case 0: r = -a; break;
      case 1: r = a + b; break;
      case 2: r = a + b.v; break;
      case 3: r = a.v + b; break;
      case 4: r = a - b; break;
      case 5: r = a - b.v; break;
      case 6: r = a.v - b; break;
      case 7: r = a * b; break;
      case 8: r = a * b.v; break;
      case 9: r = a.v * b; break;
      case 10: r = a / b; break;
      case 11: r = a / b.v; break;
      case 12: r = a.v / b; break;
      case 13: r = a; r += b; break;
      case 14: r = Dual{ta::t_val(a), 0.0}; break;
      case 15: r = ta::t_exp(a); break;
      case 16: r = ta::t_exp_libm(a); break;
      case 17: r = ta::t_log(a); break;
      case 18: r = ta::t_sqrt(a); break;
      case 19: r = ta::t_pow(a, b); break;
      case 20: r = ta::t_pow(a, b.v); break;
      case 21: r = ta::t_pow(a.v, b); break;
      case 22: r = ta::t_floor_at(a, b.v); break;
      case 256 + 0: p = -a.v; break;
      case 256 + 1: case 256 + 2: case 256 + 3: case 256 + 13: p = a.v + b.v; break;
      case 256 + 4: case 256 + 5: case 256 + 6: p = a.v - b.v; break;
      case 256 + 7: case 256 + 8: case 256 + 9: p = a.v * b.v; break;
      case 256 + 10: case 256 + 11: case 256 + 12: p = a.v / b.v; break;
      case 256 + 14: p = ta::t_val(a.v); break;
      case 256 + 15: p = ta::t_exp(a.v); break;
      case 256 + 16: p = ta::t_exp_libm(a.v); break;
      case 256 + 17: p = ta::t_log(a.v); break;
      case 256 + 18: p = ta::t_sqrt(a.v); break;
      case 256 + 19: case 256 + 20: case 256 + 21: p = ta::t_pow(a.v, b.v); break;
      case 256 + 22: p = ta::t_floor_at(a.v, b.v); break;
      default: break;
    }
    if (op >= 256) r = Dual{p, 0.0};
    y[0] = r.v;
    y[1] = r.d;
  }
};

// in: a, b, nel; out: radial_term_of(a, b), angular_term_of(a, b, nel)
struct TermIndexOp {
  static constexpr int NI = 3, NO = 2;
  __device__ void operator()(const double *x, double *y) const {
    y[0] = (double)ta::radial_term_of((int)x[0], (int)x[1]);
    y[1] = (double)ta::angular_term_of((int)x[0], (int)x[1], (int)x[2]);
  }
};

// Whole workgroups only (n is a multiple of 256), so that every lane of every wavefront takes part in
// each cross-lane step; out rows: row16_sum, group_sum<32>, wave_sum, wave_max.
__global__ __launch_bounds__(kThreads) void lane_sums_kernel(const double *in, double *out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const double v = in[i];
    out[i] = ta::row16_sum(v);
    out[(size_t)n + i] = ta::group_sum<32>(v);
    out[2 * (size_t)n + i] = ta::wave_sum(v);
    out[3 * (size_t)n + i] = ta::wave_max(v);
  }
}

}  // namespace

extern "C" {

int mp_exp(const double *in, double *out, int64_t n) { return run_map(in, out, n, ExpOp{}); }

int mp_cutoff(int kind, const double *in, double *out, int64_t n) {
  if (kind != TA_CUTOFF_COSINE && kind != TA_CUTOFF_POLYNOMIAL) return TA_ERR_INVALID;
  return run_map(in, out, n, CutoffOp{kind});
}

int mp_softplus(const double *in, double *out, int64_t n) { return run_map(in, out, n, SoftplusOp{}); }

int mp_rcp_1_3(const double *in, double *out, int64_t n) { return run_map(in, out, n, RcpOp{}); }

// any `act` outside TA_ACT_* is the linear default
int mp_activation(int act, const double *in, double *out, int64_t n) {
  return run_map(in, out, n, ActivationOp{act});
}

int mp_pow_int_m1(const double *in, double *out, int64_t n) { return run_map(in, out, n, PowIntOp{}); }

int mp_safe_pow(int safe, const double *in, double *out, int64_t n) {
  return run_map(in, out, n, SafePowOp{safe});
}

int mp_dual_ops(const double *in, double *out, int64_t n) { return run_map(in, out, n, DualOp{}); }

int mp_term_index(const double *in, double *out, int64_t n) { return run_map(in, out, n, TermIndexOp{}); }

int mp_lane_sums(const double *in, double *out, int64_t n) {
  if (!in || !out || n <= 0 || n % kThreads != 0) return TA_ERR_INVALID;
  DeviceBuf din, dout;
  const size_t bin = sizeof(double) * (size_t)n, bout = 4 * bin;
  MP_CHECK(hipMalloc(&din.p, bin));
  MP_CHECK(hipMalloc(&dout.p, bout));
  MP_CHECK(hipMemcpy(din.p, in, bin, hipMemcpyHostToDevice));
  MP_CHECK(hipMemset(dout.p, 0xff, bout));
  hipLaunchKernelGGL(lane_sums_kernel, dim3(grid_for(n)), dim3(kThreads), 0, 0, (const double *)din.p,
                     (double *)dout.p, n);
  MP_CHECK(hipGetLastError());
  MP_CHECK(hipDeviceSynchronize());
  MP_CHECK(hipMemcpy(out, dout.p, bout, hipMemcpyDeviceToHost));
  return TA_OK;
}

}  // extern "C"
