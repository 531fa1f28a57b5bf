// Element-wise and small-reduction kernels of the diffusion hot path (gfx950).
//
// Compiled with -ffp-contract=off: these kernels restate the reference's torch op sequences
// (diffusion/ddpm.py, diffusion/ddim.py), where every mul/add is a separate rounding.
//   q_sample            diffusion/ddpm.py:84-104
//   p_losses loss       diffusion/ddpm.py:130-139
//   DDPM p_sample       diffusion/ddpm.py:151-220
//   DDIM p_sample       diffusion/ddim.py:154-208
//   CFG + threshold     diffusion/ddim.py:300-325 (ddpm.py:284-303)
//   TimeEmbedding       models/unet.py:18-25
//   label embedding     models/unet.py:183, 256-258
//   EMA                 utils/trainer.py:187-202
//   clip_grad_norm_     utils/trainer.py:259
// Not in the reference: the DPM-Solver++ step (arXiv:2211.01095) and the v-prediction / min-SNR objective with its
// output conversion (arXiv:2202.00512, arXiv:2303.09556), written to the same one-rounding-per-op rule, and the
// variational-bound step of the bits-per-dimension evaluation (arXiv:2006.11239, arXiv:2102.09672), and the
// rectified-flow Euler / Heun step with its guidance kernel (arXiv:2209.03003, arXiv:2206.00364).
#include <stdlib.h>
#include <string.h>
#include "dmc_common.h"
#include "dmc_internal.h"

namespace dmc {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
}  // namespace dmc

namespace dmc {
namespace {
struct OptDef {
  const char* name;
  long def;
};
// name (= environment variable), default
constexpr OptDef kOpts[OPT_COUNT] = {
    {"DMC_NO_NARROW", 0}, {"DMC_NO_GLDS", 0}, {"DMC_NO_SPLITK", 0}, {"DMC_NO_BUFLDS", 0}, {"DMC_NO_HALO", 0},
    {"DMC_HALO_PRO", 1}, {"DMC_GN_STATS_SPLIT", 0}, {"DMC_GN_BWD_SPLIT", 0}, {"DMC_ATTN_STAGED", 0},
    {"DMC_ATTN_HG", 0}, {"DMC_WG_BLOCKS", 512}, {"DMC_GN_STATS_ONE_MAX", 1l << 20}, {"DMC_GN_BWD_ONE_MAX", 65536},
    {"DMC_NO_XCD", 0}, {"DMC_NO_EPI_STATS", 0}, {"DMC_WG_MINPIX", 0}, {"DMC_GN_BWD_SLICES", 2}, {"DMC_NO_SKGN", 0},
    {"DMC_WG_HALO_TARGET", 256}, {"DMC_SK_TARGET", 240}, {"DMC_NO_NHALO", 0},
    {"DMC_GN_BWD_FUSED", 4}, {"DMC_GEMM1X1_WK", 1}, {"DMC_GN_BWD_NT", 1024},
    {"DMC_REG_EPI", 3}, {"DMC_GEMM1X1", 1}, {"DMC_WG_PIPE", 1}, {"DMC_IMG_MASK", 15}, {"DMC_IMG_GN", 1}, {"DMC_WG_IMG4", 1},
    {"DMC_RESAMPLE_FOLD", 1},
};
struct OptTable {
  long v[OPT_COUNT];
  OptTable() { reset(true); }
  void reset(bool env) {
    for (int i = 0; i < OPT_COUNT; ++i) {
      v[i] = kOpts[i].def;
      const char* e = env ? getenv(kOpts[i].name) : nullptr;
      if (e && e[0]) v[i] = atol(e);
    }
  }
};
OptTable& table() {
  static OptTable t;   // thread-safe one-time initialisation from the environment
  return t;
}
}  // namespace
long opt(Opt o) { return table().v[o]; }
}  // namespace dmc

extern "C" int dmc_set_option(const char* name, long value) {
  for (int i = 0; i < dmc::OPT_COUNT; ++i)
    if (strcmp(name, dmc::kOpts[i].name) == 0) {
      dmc::table().v[i] = value;
      return 0;
    }
  dmc::set_error("set_option: unknown option %s", name);
  return 1;
}
extern "C" long dmc_get_option(const char* name) {
  for (int i = 0; i < dmc::OPT_COUNT; ++i)
    if (strcmp(name, dmc::kOpts[i].name) == 0) return dmc::table().v[i];
  return -1;
}
extern "C" void dmc_reset_options(int from_env) { dmc::table().reset(from_env != 0); }

extern "C" int dmc_version(void) { return 1; }
extern "C" const char* dmc_last_error(void) { return dmc::g_err; }

namespace {

inline int grid_for(long n, int block = 256, int cap = 8192) {
  long b = (n + block - 1) / block;
  if (b < 1) b = 1;
  return (int)(b < cap ? b : cap);
}

__global__ void time_embed_kernel(const int64_t* t, int B, int dim, float* out) {
  const int half = dim / 2;
  const float e = (float)(9.210340371976184 / (double)(half - 1));  // math.log(10000)/(half-1)
  const int total = B * half;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / half, k = i % half;
    const float f = expf((float)k * -e);
    const float a = (float)t[b] * f;
    out[(size_t)b * dim + k] = sinf(a);
    out[(size_t)b * dim + half + k] = cosf(a);
  }
}

__global__ void embed_fwd_kernel(const int64_t* y, int B, int rows, const float* table, int dim, float* out) {
  const int total = B * dim;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int b = i / dim, d = i % dim;
    long yy = y[b];
    yy = yy < 0 ? 0 : (yy > rows - 1 ? rows - 1 : yy);
    out[i] = table[(size_t)yy * dim + d];
  }
}

// dtable[row][d] = sum_{b: clamp(y_b) == row} dout[b][d] in batch order; row 0 (padding_idx) gets 0
__global__ void embed_bwd_kernel(const int64_t* y, int B, int rows, const float* dout, int dim, float* dtable) {
  const int total = rows * dim;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int r = i / dim, d = i % dim;
    float s = 0.f;
    if (r != 0) {
      for (int b = 0; b < B; ++b) {
        long yy = y[b];
        yy = yy < 0 ? 0 : (yy > rows - 1 ? rows - 1 : yy);
        if (yy == r) s += dout[(size_t)b * dim + d];
      }
    }
    dtable[i] = s;
  }
}

template <typename T>
__global__ void pack_input_kernel(const float* x, const float* noise, const int64_t* t, const float* a, const float* b,
                                  int N, int C, int H, int W, T* dst, int ld) {
  const long total = (long)N * H * W * ld;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = i % ld;
    const long pix = i / ld;
    const int n = pix / (H * W);
    const int hw = pix % (H * W);
    float v = 0.f;
    if (c < C) {
      const size_t src = ((size_t)n * C + c) * H * W + hw;
      v = x[src];
      if (t) {
        const float an = a[t[n]], bn = b[t[n]];
        v = an * v + bn * noise[src];
      }
    }
    if (sizeof(T) == 4) ((float*)dst)[i] = v;
    else ((bf16_t*)dst)[i] = (bf16_t)f2bf(v);
  }
}

__global__ void q_sample_kernel(const float* x0, const float* noise, const int64_t* t, const float* a, const float* b,
                                long total, int per, float* out) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int n = i / per;
    const float an = a[t[n]], bn = b[t[n]];
    const float u = an * x0[i];
    const float v = bn * noise[i];
    out[i] = u + v;
  }
}

// ---------------- loss ----------------
__device__ __forceinline__ float loss_elem(int type, float d) {
  if (type == DMC_LOSS_L2) return d * d;
  if (type == DMC_LOSS_L1) return fabsf(d);
  const float ad = fabsf(d);
  return ad < 1.f ? 0.5f * d * d : ad - 0.5f;
}

__global__ __launch_bounds__(256) void loss_partial_kernel(int type, const float* pred, const float* target, long n,
                                                           float* partial) {
  float s = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    s += loss_elem(type, target[i] - pred[i]);
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void loss_final_kernel(const float* partial, int nb, long n, float* loss) {
  __shared__ float red[4];
  float s = 0.f;
  for (int i = threadIdx.x; i < nb; i += blockDim.x) s += partial[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) loss[0] = ((red[0] + red[1]) + (red[2] + red[3])) / (float)n;
}

__global__ void loss_bwd_kernel(int type, const float* pred, const float* target, long n, const float* dloss,
                                float* dpred) {
  const float g = dloss[0] / (float)n;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float d = pred[i] - target[i];
    float v;
    if (type == DMC_LOSS_L2) v = 2.f * d;
    else if (type == DMC_LOSS_L1) v = (d > 0.f) ? 1.f : (d < 0.f ? -1.f : 0.f);
    else v = fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : -1.f);
    dpred[i] = v * g;
  }
}

// ---------------- objective: prediction target, per-sample weight, loss and gradient in one pass ----------------
// v-prediction target (Salimans & Ho 2022, arXiv:2202.00512, eq. 31 / appendix D): v = alpha*eps - sigma*x0; min-SNR
// weights (Hang et al. 2023, arXiv:2303.09556) come from the host as a [T] table (diffusion/_objective.py). One
// element: target, the loss term of loss_partial_kernel and, when a gradient is asked for, loss_bwd_kernel's value;
// every op is a separate rounding.
DMC_DEV float obj_target(int pred_type, float sa, float s1, float x0, float e) {
  if (pred_type != DMC_PRED_V) return e;
  const float a_ = sa * e;
  const float b_ = s1 * x0;
  return a_ - b_;
}

DMC_DEV float obj_elem(int pred_type, int type, float sa, float s1, float p, float x0, float e, bool grad, float scale,
                       float& dp) {
  const float target = obj_target(pred_type, sa, s1, x0, e);
  if (grad) {
    const float d = p - target;
    float v;
    if (type == DMC_LOSS_L2) v = 2.f * d;
    else if (type == DMC_LOSS_L1) v = (d > 0.f) ? 1.f : (d < 0.f ? -1.f : 0.f);
    else v = fabsf(d) < 1.f ? d : (d > 0.f ? 1.f : -1.f);
    dp = v * scale;
  }
  return loss_elem(type, target - p);
}

DMC_DEV long clamp_t(long t, int T) { return t < 0 ? 0 : (t > T - 1 ? T - 1 : t); }   // never index past a table

// Grid as dpm_step_kernel: blockIdx.y strides over samples, blockIdx.x over the sample's elements, so t and the
// table entries are block-uniform, read once per sample. Block (bx, n) leaves its sum at partial[n * gridDim.x + bx];
// pred / x0 / noise are read once and dpred written once in that same pass. x0 is read for v-prediction only.
// IS (dmc_objective_is with a table): iw[t_n] is the sample's importance weight, the gradient's LAST factor, so dpred is
// iw[t_n] times dmc_objective's dpred rounded once, and with 1 its bits. Without IS iw is unread and the code is
// dmc_objective's as it was.
template <bool VEC, bool IS>
__global__ __launch_bounds__(256) void objective_kernel(int pred_type, int type, const float* pred, const float* x0,
                                                        const float* noise, const int64_t* t, const float* sa,
                                                        const float* s1, const float* w, const float* iw, int T,
                                                        int N, int per, const float* dloss, float* dpred,
                                                        float* partial) {
  __shared__ float red[4];
  const bool grad = dpred != nullptr;
  const bool isv = pred_type == DMC_PRED_V;
  const float g = grad ? dloss[0] / (float)((long)N * per) : 0.f;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const long tt = clamp_t(t[n], T);
    const float san = isv ? sa[tt] : 0.f, s1n = isv ? s1[tt] : 0.f;
    float scale = g;
    if (w) scale = g * w[tt];
    const float iwn = IS ? iw[tt] : 1.f;
    const size_t base = (size_t)n * per;
    float s = 0.f;
    if (VEC) {
      const int per4 = per / 4;
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per4; q += gridDim.x * blockDim.x) {
        const size_t i = base + (size_t)q * 4;
        const v4f pv = *(const v4f*)(pred + i);
        const v4f ev = *(const v4f*)(noise + i);
        v4f xv = {0.f, 0.f, 0.f, 0.f}, dv = xv;
        if (isv) xv = *(const v4f*)(x0 + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float dp = 0.f;
          s += obj_elem(pred_type, type, san, s1n, pv[k], xv[k], ev[k], grad, scale, dp);
          dv[k] = IS ? dp * iwn : dp;
        }
        if (grad) *(v4f*)(dpred + i) = dv;
      }
    } else {
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per; q += gridDim.x * blockDim.x) {
        const size_t i = base + q;
        float dp = 0.f;
        s += obj_elem(pred_type, type, san, s1n, pred[i], isv ? x0[i] : 0.f, noise[i], grad, scale, dp);
        if (grad) dpred[i] = IS ? dp * iwn : dp;
      }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)n * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();   // red is reused by the block's next sample
  }
}

// loss = (1/N) sum_n w[t_n] * (1/per) * (sample n's partials in block order), samples added in index order by one
// thread: a fixed order, no atomics. dmc_objective_is: row_loss[n] (if given) is sample n's term of that sum, and the
// term enters the sum times iw[t_n] (NULL: as it is).
__global__ __launch_bounds__(256) void objective_final_kernel(const float* partial, int gx, const int64_t* t,
                                                              const float* w, const float* iw, int T, int N, int per,
                                                              float* loss, float* row_loss) {
  __shared__ float sm[256];
  float total = 0.f;
  for (int n0 = 0; n0 < N; n0 += 256) {
    const int n = n0 + threadIdx.x;
    float m = 0.f;
    if (n < N) {
      float s = 0.f;
      for (int b = 0; b < gx; ++b) s += partial[(size_t)n * gx + b];
      m = s / (float)per;
      if (w) m = w[clamp_t(t[n], T)] * m;
      if (row_loss) row_loss[n] = m;
      if (iw) m = iw[clamp_t(t[n], T)] * m;
    }
    sm[threadIdx.x] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int cnt = N - n0 < 256 ? N - n0 : 256;
      for (int k = 0; k < cnt; ++k) total += sm[k];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = total / (float)N;
}

// v-prediction model output -> (eps, x0) for the step kernels; row r*N + n of pred pairs with x[n], t[n] (reps = 2:
// the batched cond / uncond forward of CFG). x0 is formed directly, with no division by alpha.
template <bool VEC>
__global__ __launch_bounds__(256) void pred_convert_kernel(const float* x, const int64_t* t, const float* sa,
                                                           const float* s1, int T, const float* pred, int reps,
                                                           int N, int per, float* eps_out, float* x0_out) {
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const long tt = clamp_t(t[n], T);
    const float san = sa[tt], s1n = s1[tt];
    const size_t xbase = (size_t)n * per;
    for (int r = 0; r < reps; ++r) {
      const size_t base = ((size_t)r * N + n) * per;
      if (VEC) {
        const int per4 = per / 4;
        for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per4; q += gridDim.x * blockDim.x) {
          const v4f xv = *(const v4f*)(x + xbase + (size_t)q * 4);
          const v4f pv = *(const v4f*)(pred + base + (size_t)q * 4);
          v4f ev, x0v;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float u = s1n * xv[k];
            const float qq = san * pv[k];
            ev[k] = u + qq;
            const float p = san * xv[k];
            const float rr = s1n * pv[k];
            x0v[k] = p - rr;
          }
          *(v4f*)(eps_out + base + (size_t)q * 4) = ev;
          if (x0_out) *(v4f*)(x0_out + base + (size_t)q * 4) = x0v;
        }
      } else {
        for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per; q += gridDim.x * blockDim.x) {
          const float xx = x[xbase + q], pp = pred[base + q];
          const float u = s1n * xx;
          const float qq = san * pp;
          eps_out[base + q] = u + qq;
          if (x0_out) {
            const float p = san * xx;
            const float rr = s1n * pp;
            x0_out[base + q] = p - rr;
          }
        }
      }
    }
  }
}

// ---------------- variational bound (bits per dimension): one timestep's terms and the next x_t in one pass ----------------
// Ho et al. 2020 (arXiv:2006.11239 §3-4), Nichol & Dhariwal 2021 (arXiv:2102.09672 §2-3); the host table is
// diffusion/_vlb.py: row {c_x, c_p, kprec, kvar, keps, isig}. The KL of the two posteriors is kvar + kprec*(x0 - x0_pred)^2:
// their means differ by c1*(x0 - x0_pred) exactly and are never formed (formed first they cancel at the noisy end).
struct VlbRow {
  float cx, cp, kprec, kvar, isig;
};

// Exact normal CDF (not the tanh approximation of some public implementations).
DMC_DEV float vlb_cdf(float z) { return 0.5f * erfcf(-z * 0.70710678118654752f); }

DMC_DEV float vlb_zpdf(float z) { return z * (0.39894228040143268f * expf(-0.5f * z * z)); }   // z * phi(z)

// -log p of one element under the decoder's Gaussian discretised on the 8-bit grid k/127.5 - 1; d = x0 - mean.
// GRAD: dlv = d(-log p) / d(log variance), with isig = exp(-0.5 log variance): dz/dlv = -z/2 for both z, so
// dlv = 0.5 (zp phi(zp) - zm phi(zm)) / p with the absent edge's term dropped, and 0 where the floor acts (as clamp
// gives under autograd).
template <bool GRAD>
DMC_DEV float vlb_decoder_g(float x0, float d, float isig, float& dlv) {
  const float h = 1.0f / 255.0f;
  const float zp = (d + h) * isig;
  const float zm = (d - h) * isig;
  float pr, num = 0.f;
  if (x0 < -0.999f) {
    pr = vlb_cdf(zp);
    if (GRAD) num = vlb_zpdf(zp);
  } else if (x0 > 0.999f) {
    pr = vlb_cdf(-zm);
    if (GRAD) num = -vlb_zpdf(zm);
  } else {
    if (zm <= 0.f) pr = vlb_cdf(zp) - vlb_cdf(zm);
    else pr = vlb_cdf(-zm) - vlb_cdf(-zp);      // both values below 1/2: the difference keeps its digits
    if (GRAD) num = vlb_zpdf(zp) - vlb_zpdf(zm);
  }
  if (GRAD) dlv = pr >= 1e-12f ? 0.5f * num / pr : 0.f;
  return -logf(fmaxf(pr, 1e-12f));
}

DMC_DEV float vlb_decoder(float x0, float d, float isig) {
  float unused;
  return vlb_decoder_g<false>(x0, d, isig, unused);
}

struct VlbSums {
  float term, dd, du, xx;
};

// u = c_x*x_t - c_p*pred is the x0 prediction as fp32 holds it. x0 - u is formed without u's rounding, as
// (x0 - c_x*x_t) + c_p*pred plus the two products' rounding errors (exact, by fma): where the prediction is good the
// difference is small against x0 and would otherwise keep only its leading digits.
DMC_DEV void vlb_delta(float cx, float cp, int clip, float x0, float xt, float p, float& d, float& du) {
  const float a_ = cx * xt;
  const float ae = fmaf(cx, xt, -a_);
  const float b_ = cp * p;
  const float be = fmaf(cp, p, -b_);
  const float u = a_ - b_;
  du = ((x0 - a_) + b_) + (be - ae);
  d = du;
  if (clip && u > 1.f) d = x0 - 1.f;
  if (clip && u < -1.f) d = x0 + 1.f;
}

DMC_DEV void vlb_elem(const VlbRow& r, bool dec, int clip, float x0, float xt, float p, VlbSums& s) {
  float d, du;
  vlb_delta(r.cx, r.cp, clip, x0, xt, p, d, du);
  const float d2 = d * d;
  s.term += dec ? vlb_decoder(x0, d, r.isig) : r.kvar + r.kprec * d2;
  s.dd += d2;
  s.du += du * du;
  s.xx += x0 * x0;
}

// Grid as objective_kernel: blockIdx.y strides over samples, blockIdx.x over the sample's elements, so t, the row and
// the decoder branch are block-uniform. Block (bx, n) leaves its four sums at partial[(n * gridDim.x + bx) * 4 ..].
// x0, x_t and pred are read once; with x_next, z_next is read and x_next written in the same pass (dmc_q_sample's ops).
template <bool VEC>
__global__ __launch_bounds__(256) void vlb_step_kernel(const float* x0, const float* xt, const float* pred,
                                                       const int64_t* t, const float* coef, int T, int clip,
                                                       const float* zn, const int64_t* t_next, const float* sa,
                                                       const float* s1, int N, int per, float* x_next,
                                                       float* partial) {
  __shared__ float red[4][4];
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const long tt = clamp_t(t[n], T);
    const float* c = coef + tt * 6;
    const VlbRow r{c[0], c[1], c[2], c[3], c[5]};
    const bool dec = tt == 0;
    bool fwd = false;
    float an = 0.f, bn = 0.f;
    if (x_next != nullptr && t_next[n] >= 0) {
      const long tn = clamp_t(t_next[n], T);
      fwd = true;
      an = sa[tn];
      bn = s1[tn];
    }
    const size_t base = (size_t)n * per;
    VlbSums s{0.f, 0.f, 0.f, 0.f};
    if (VEC) {
      const int per4 = per / 4;
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per4; q += gridDim.x * blockDim.x) {
        const size_t i = base + (size_t)q * 4;
        const v4f xv = *(const v4f*)(x0 + i);
        const v4f tv = *(const v4f*)(xt + i);
        const v4f pv = *(const v4f*)(pred + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) vlb_elem(r, dec, clip, xv[k], tv[k], pv[k], s);
        if (fwd) {
          const v4f zv = *(const v4f*)(zn + i);
          v4f ov;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float u = an * xv[k];
            const float v = bn * zv[k];
            ov[k] = u + v;
          }
          *(v4f*)(x_next + i) = ov;
        }
      }
    } else {
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per; q += gridDim.x * blockDim.x) {
        const size_t i = base + q;
        const float xx = x0[i];
        vlb_elem(r, dec, clip, xx, xt[i], pred[i], s);
        if (fwd) {
          const float u = an * xx;
          const float v = bn * zn[i];
          x_next[i] = u + v;
        }
      }
    }
    float v[4] = {wave_sum(s.term), wave_sum(s.dd), wave_sum(s.du), wave_sum(s.xx)};
    if ((threadIdx.x & 63) == 0)
      for (int k = 0; k < 4; ++k) red[k][threadIdx.x >> 6] = v[k];
    __syncthreads();
    if (threadIdx.x < 4) {
      const float* rk = red[threadIdx.x];
      partial[((size_t)n * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = (rk[0] + rk[1]) + (rk[2] + rk[3]);
    }
    __syncthreads();   // red is reused by the block's next sample
  }
}

// Thread n adds sample n's partials in block order: a fixed order, no atomics.
// keps is column keps_col of the table's cols-wide rows.
__global__ __launch_bounds__(256) void vlb_final_kernel(const float* partial, int gx, const int64_t* t,
                                                        const float* coef, int cols, int keps_col, int T, int N,
                                                        int per, float* vb, float* xstart_mse, float* eps_mse,
                                                        float* x0_sq) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int b = 0; b < gx; ++b)
    for (int k = 0; k < 4; ++k) s[k] += partial[((size_t)n * gx + b) * 4 + k];
  const float keps = coef[clamp_t(t[n], T) * cols + keps_col];
  const float fp = (float)per;
  vb[n] = (s[0] / fp) / 0.69314718055994531f;
  xstart_mse[n] = s[1] / fp;
  eps_mse[n] = keps * (s[2] / fp);
  x0_sq[n] = s[3] / fp;
}

// ---------------- learned variances: hybrid loss, bound step and sampler step ----------------
// Nichol & Dhariwal 2021 (arXiv:2102.09672 §3.1, eq. 15-16): the network's second half v interpolates the log-variance
// between the posterior's (lv_min) and beta's: lv_p = lv_min + d, d = (v + 1)/2 * R, R = lv_max - lv_min, not clamped.
// The host table is diffusion/_vlb.py learned_coefficients: row {c_x, c_p, c1, lv_min, R, kmin, keps, lv_max}. With
// delta = x0 - x0_pred (the means differ by c1*delta and are never formed) the KL against the true posterior is
//   0.5 (d + expm1(-d)) + kmin exp(-d) delta^2,   kmin = 0.5 c1^2 exp(-lv_min)
// in the expm1 form: R falls to 8e-7 at the noisy end, where -1 + d + exp(-d) is exactly 0 in fp32.
struct LvarRow {
  float lvmin, R, kmin;
};

DMC_DEV LvarRow lvar_row(const float* coef, long tt) {
  const float* c = coef + tt * DMC_LVAR_COLS;
  return LvarRow{c[3], c[4], c[5]};
}

DMC_DEV float lvar_d(const LvarRow& r, float v) {
  const float frac = (v + 1.f) * 0.5f;
  return frac * r.R;
}

// The term of one element (KL for t >= 1, the decoder's -log p for t = 0: dec), in nats; GRAD: dv = d term / d v.
// The one function behind dmc_hybrid_objective, dmc_vlb_step_learned and (lvar_d) dmc_ddpm_step_learned.
template <bool GRAD>
DMC_DEV float lvar_term(const LvarRow& r, bool dec, float x0, float delta, float v, float& dv) {
  const float d = lvar_d(r, v);
  const float hr = 0.5f * r.R;                  // d lv_p / d v
  if (dec) {
    const float isig = expf(-0.5f * (r.lvmin + d));
    float dlv = 0.f;
    const float term = vlb_decoder_g<GRAD>(x0, delta, isig, dlv);
    if (GRAD) dv = dlv * hr;
    return term;
  }
  const float em = expm1f(-d);
  const float q = (r.kmin * (1.f + em)) * (delta * delta);
  if (GRAD) dv = (-0.5f * em - q) * hr;
  return 0.5f * (d + em) + q;
}

// objective_kernel over out = [N][2][per]: the prediction half goes through obj_elem unchanged (so L_simple and its
// gradient keep dmc_objective's bits), the v half gets the term with delta = c_p*(pred - target), which needs neither
// x_t nor a division. The term sends no gradient to the prediction half. Block (bx, n) leaves {simple, term} sums at
// partial[(n * gridDim.x + bx) * 2 ..]. x0 is read where the sample needs it: v-prediction, or t = 0 (the edges).
// IS and iw as in objective_kernel: the last factor of both halves' gradient.
template <bool VEC, bool GRAD, bool IS>
__global__ __launch_bounds__(256) void hybrid_objective_kernel(int pred_type, int type, const float* out,
                                                               const float* x0, const float* noise, const int64_t* t,
                                                               const float* sa, const float* s1, const float* w,
                                                               const float* iw, const float* coef, int T, int N, int per,
                                                               float vlb_weight, const float* dloss, float* dout,
                                                               float* partial) {
  __shared__ float red[2][4];
  const bool isv = pred_type == DMC_PRED_V;
  const float g = GRAD ? dloss[0] / (float)((long)N * per) : 0.f;
  const float gv = (g * vlb_weight) / 0.69314718055994531f;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const long tt = clamp_t(t[n], T);
    const float san = isv ? sa[tt] : 0.f, s1n = isv ? s1[tt] : 0.f;
    const float cp = coef[tt * DMC_LVAR_COLS + 1];
    const LvarRow r = lvar_row(coef, tt);
    const bool dec = tt == 0, rdx = isv || dec;
    float scale = g;
    if (w) scale = g * w[tt];
    const float iwn = IS ? iw[tt] : 1.f;
    const size_t xbase = (size_t)n * per, obase = 2 * xbase;
    float ss = 0.f, sv = 0.f;
    if (VEC) {
      const int per4 = per / 4;
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per4; q += gridDim.x * blockDim.x) {
        const size_t i = xbase + (size_t)q * 4, o = obase + (size_t)q * 4;
        const v4f pv = *(const v4f*)(out + o);
        const v4f vv = *(const v4f*)(out + o + per);
        const v4f ev = *(const v4f*)(noise + i);
        v4f xv = {0.f, 0.f, 0.f, 0.f}, dpv = xv, dvv = xv;
        if (rdx) xv = *(const v4f*)(x0 + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float dp = 0.f, dv = 0.f;
          ss += obj_elem(pred_type, type, san, s1n, pv[k], xv[k], ev[k], GRAD, scale, dp);
          const float delta = cp * (pv[k] - obj_target(pred_type, san, s1n, xv[k], ev[k]));
          sv += lvar_term<GRAD>(r, dec, xv[k], delta, vv[k], dv);
          dpv[k] = IS ? dp * iwn : dp;
          dvv[k] = IS ? (gv * dv) * iwn : gv * dv;
        }
        if (GRAD) {
          *(v4f*)(dout + o) = dpv;
          *(v4f*)(dout + o + per) = dvv;
        }
      }
    } else {
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per; q += gridDim.x * blockDim.x) {
        const size_t i = xbase + q, o = obase + q;
        const float p = out[o], xx = rdx ? x0[i] : 0.f, e = noise[i];
        float dp = 0.f, dv = 0.f;
        ss += obj_elem(pred_type, type, san, s1n, p, xx, e, GRAD, scale, dp);
        const float delta = cp * (p - obj_target(pred_type, san, s1n, xx, e));
        sv += lvar_term<GRAD>(r, dec, xx, delta, out[o + per], dv);
        if (GRAD) {
          dout[o] = IS ? dp * iwn : dp;
          dout[o + per] = IS ? (gv * dv) * iwn : gv * dv;
        }
      }
    }
    ss = wave_sum(ss);
    sv = wave_sum(sv);
    if ((threadIdx.x & 63) == 0) {
      red[0][threadIdx.x >> 6] = ss;
      red[1][threadIdx.x >> 6] = sv;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      const float* rk = red[threadIdx.x];
      partial[((size_t)n * gridDim.x + blockIdx.x) * 2 + threadIdx.x] = (rk[0] + rk[1]) + (rk[2] + rk[3]);
    }
    __syncthreads();   // red is reused by the block's next sample
  }
}

// objective_final_kernel's order for both sums: loss = {simple + vlb, simple, vlb}, simple as dmc_objective's loss[0],
// vlb = vlb_weight * (1/N) sum_n (1/per) * (sample n's term partials in block order) / ln 2.
// dmc_hybrid_objective_is: row_loss[n] = simple_n + vlb_weight * vb_n of the two per-sample terms, which enter their sums
// times iw[t_n] (NULL: as they are).
__global__ __launch_bounds__(256) void hybrid_final_kernel(const float* partial, int gx, const int64_t* t,
                                                           const float* w, const float* iw, int T, int N, int per,
                                                           float vlb_weight, float* loss, float* row_loss) {
  __shared__ float sm[2][256];
  float total = 0.f, totalv = 0.f;
  for (int n0 = 0; n0 < N; n0 += 256) {
    const int n = n0 + threadIdx.x;
    float m = 0.f, mv = 0.f;
    if (n < N) {
      float s = 0.f, sv = 0.f;
      for (int b = 0; b < gx; ++b) {
        s += partial[((size_t)n * gx + b) * 2];
        sv += partial[((size_t)n * gx + b) * 2 + 1];
      }
      m = s / (float)per;
      if (w) m = w[clamp_t(t[n], T)] * m;
      mv = (sv / (float)per) / 0.69314718055994531f;
      if (row_loss) row_loss[n] = m + vlb_weight * mv;
      if (iw) {
        const float iwn = iw[clamp_t(t[n], T)];
        m = iwn * m;
        mv = iwn * mv;
      }
    }
    sm[0][threadIdx.x] = m;
    sm[1][threadIdx.x] = mv;
    __syncthreads();
    if (threadIdx.x == 0) {
      const int cnt = N - n0 < 256 ? N - n0 : 256;
      for (int k = 0; k < cnt; ++k) {
        total += sm[0][k];
        totalv += sm[1][k];
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float simple = total / (float)N;
    const float vlb = vlb_weight * (totalv / (float)N);
    loss[0] = simple + vlb;
    loss[1] = simple;
    loss[2] = vlb;
  }
}

// vlb_step_kernel with the learned term: pred and v are rows of the model's [N][2][per] output, read in place through
// their row strides.
template <bool VEC>
__global__ __launch_bounds__(256) void vlb_step_learned_kernel(const float* x0, const float* xt, const float* pred,
                                                               long pred_ld, const float* v, long v_ld,
                                                               const int64_t* t, const float* coef, int T, int clip,
                                                               const float* zn, const int64_t* t_next,
                                                               const float* sa, const float* s1, int N, int per,
                                                               float* x_next, float* partial) {
  __shared__ float red[4][4];
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const long tt = clamp_t(t[n], T);
    const float cx = coef[tt * DMC_LVAR_COLS], cp = coef[tt * DMC_LVAR_COLS + 1];
    const LvarRow r = lvar_row(coef, tt);
    const bool dec = tt == 0;
    bool fwd = false;
    float an = 0.f, bn = 0.f;
    if (x_next != nullptr && t_next[n] >= 0) {
      const long tn = clamp_t(t_next[n], T);
      fwd = true;
      an = sa[tn];
      bn = s1[tn];
    }
    const size_t base = (size_t)n * per;
    const float* pn = pred + (size_t)n * pred_ld;
    const float* vn = v + (size_t)n * v_ld;
    VlbSums s{0.f, 0.f, 0.f, 0.f};
    float unused;
    if (VEC) {
      const int per4 = per / 4;
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per4; q += gridDim.x * blockDim.x) {
        const size_t i = base + (size_t)q * 4;
        const v4f xv = *(const v4f*)(x0 + i);
        const v4f tv = *(const v4f*)(xt + i);
        const v4f pv = *(const v4f*)(pn + (size_t)q * 4);
        const v4f vv = *(const v4f*)(vn + (size_t)q * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float d, du;
          vlb_delta(cx, cp, clip, xv[k], tv[k], pv[k], d, du);
          s.term += lvar_term<false>(r, dec, xv[k], d, vv[k], unused);
          s.dd += d * d;
          s.du += du * du;
          s.xx += xv[k] * xv[k];
        }
        if (fwd) {
          const v4f zv = *(const v4f*)(zn + i);
          v4f ov;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float u = an * xv[k];
            const float w_ = bn * zv[k];
            ov[k] = u + w_;
          }
          *(v4f*)(x_next + i) = ov;
        }
      }
    } else {
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per; q += gridDim.x * blockDim.x) {
        const size_t i = base + q;
        const float xx = x0[i];
        float d, du;
        vlb_delta(cx, cp, clip, xx, xt[i], pn[q], d, du);
        s.term += lvar_term<false>(r, dec, xx, d, vn[q], unused);
        s.dd += d * d;
        s.du += du * du;
        s.xx += xx * xx;
        if (fwd) {
          const float u = an * xx;
          const float w_ = bn * zn[i];
          x_next[i] = u + w_;
        }
      }
    }
    float sums[4] = {wave_sum(s.term), wave_sum(s.dd), wave_sum(s.du), wave_sum(s.xx)};
    if ((threadIdx.x & 63) == 0)
      for (int k = 0; k < 4; ++k) red[k][threadIdx.x >> 6] = sums[k];
    __syncthreads();
    if (threadIdx.x < 4) {
      const float* rk = red[threadIdx.x];
      partial[((size_t)n * gridDim.x + blockIdx.x) * 4 + threadIdx.x] = (rk[0] + rk[1]) + (rk[2] + rk[3]);
    }
    __syncthreads();   // red is reused by the block's next sample
  }
}

// ddpm_step_kernel's ops with the learned standard deviation exp(0.5 (lv_min + d)); eps and v are rows of the model
// output read in place. Grid as dpm_step_kernel: t and the table entries are block-uniform.
DMC_DEV float ddpm_learned_elem(float a, float b, float k1, float k2, int clip, bool from_eps, float x, float e,
                                float x0, bool nz, const LvarRow& r, float v, float z) {
  if (from_eps) {
    const float u = a * x;
    const float w_ = b * e;
    x0 = u - w_;
  }
  if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
  const float m1 = k1 * x0;
  const float m2 = k2 * x;
  const float mean = m1 + m2;
  if (!nz) return mean;
  const float sd = expf(0.5f * (r.lvmin + lvar_d(r, v)));
  return mean + sd * z;
}

template <bool VEC>
__global__ __launch_bounds__(256) void ddpm_step_learned_kernel(const float* x, const float* eps, long eps_ld,
                                                                const float* v, long v_ld, const float* x0_in,
                                                                const int64_t* t, const float* sra, const float* srm1,
                                                                const float* c1, const float* c2, const float* coef,
                                                                int T, int N, int per, int clip, const float* z,
                                                                float* out) {
  const bool from_eps = x0_in == nullptr;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    const long tt = clamp_t(t[n], T);
    const float a = from_eps ? sra[tt] : 0.f, b = from_eps ? srm1[tt] : 0.f, k1 = c1[tt], k2 = c2[tt];
    const LvarRow r = lvar_row(coef, tt);
    const bool nz = z != nullptr && tt != 0;
    const size_t base = (size_t)n * per;
    const float* en = from_eps ? eps + (size_t)n * eps_ld : nullptr;
    const float* vn = nz ? v + (size_t)n * v_ld : nullptr;
    if (VEC) {
      const int per4 = per / 4;
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per4; q += gridDim.x * blockDim.x) {
        const size_t i = base + (size_t)q * 4;
        const v4f zero = {0.f, 0.f, 0.f, 0.f};
        const v4f xv = *(const v4f*)(x + i);
        const v4f ev = from_eps ? *(const v4f*)(en + (size_t)q * 4) : zero;
        const v4f x0v = from_eps ? zero : *(const v4f*)(x0_in + i);
        const v4f vv = nz ? *(const v4f*)(vn + (size_t)q * 4) : zero;
        const v4f zv = nz ? *(const v4f*)(z + i) : zero;
        v4f ov;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          ov[k] = ddpm_learned_elem(a, b, k1, k2, clip, from_eps, xv[k], ev[k], x0v[k], nz, r, vv[k], zv[k]);
        *(v4f*)(out + i) = ov;
      }
    } else {
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per; q += gridDim.x * blockDim.x) {
        const size_t i = base + q;
        out[i] = ddpm_learned_elem(a, b, k1, k2, clip, from_eps, x[i], from_eps ? en[q] : 0.f,
                                   from_eps ? 0.f : x0_in[i], nz, r, nz ? vn[q] : 0.f, nz ? z[i] : 0.f);
      }
    }
  }
}

// ---------------- samplers ----------------
__global__ void ddim_step_kernel(const float* x, const float* eps, const float* x0_in, const int64_t* t,
                                 const int64_t* t_next, const float* ac, int N, int per, float eta, int clip,
                                 const float* z, float* out) {
  // the final step of the loop (ddim.py:196-200: t_next < 0 for the batch): the block's threads test the entries
  // in parallel (a single thread walking them serialised N dependent-latency loads in every block)
  int neg = 0;
  for (int b = threadIdx.x; b < N; b += blockDim.x) neg |= (t_next[b] < 0);
  const int any_neg = __syncthreads_or(neg);
  const long total = (long)N * per;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int n = i / per;
    const float at = ac[t[n]];
    const float an = any_neg ? 1.0f : ac[t_next[n]];
    const float e = eps[i];
    float x0;
    if (x0_in) x0 = x0_in[i];
    else {
      const float s1 = sqrtf(1.0f - at);
      const float num = x[i] - s1 * e;
      x0 = num / sqrtf(at);
    }
    if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    float sigma = 0.f;
    {
      const float r1 = (1.0f - an) / (1.0f - at);
      const float r2 = 1.0f - at / an;
      float v = r1 * r2;
      v = v < 0.f ? 0.f : v;
      sigma = eta * sqrtf(v);
    }
    float c = 1.0f - an;
    c = c - sigma * sigma;
    c = c < 0.f ? 0.f : c;
    const float dir = sqrtf(c) * e;
    float xp = sqrtf(an) * x0;
    xp = xp + dir;
    if (eta > 0.f && z) xp = xp + sigma * z[i];
    out[i] = xp;
  }
}

__global__ void ddpm_step_kernel(const float* x, const float* eps, const float* x0_in, const int64_t* t,
                                 const float* sra, const float* srm1, const float* c1, const float* c2,
                                 const float* lv, int N, int per, int clip, const float* z, float* out) {
  const long total = (long)N * per;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int n = i / per;
    const long tt = t[n];
    float x0;
    if (x0_in) x0 = x0_in[i];
    else {
      const float u = sra[tt] * x[i];
      const float v = srm1[tt] * eps[i];
      x0 = u - v;
    }
    if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
    const float m1 = c1[tt] * x0;
    const float m2 = c2[tt] * x[i];
    const float mean = m1 + m2;
    const float mask = tt != 0 ? 1.0f : 0.0f;
    const float sd = expf(0.5f * lv[tt]);
    float o = mean;
    if (z) o = mean + (mask * sd) * z[i];
    out[i] = o;
  }
}

// DPM-Solver++ multistep update in data-prediction form (diffusion/_dpm.py builds the coefficient rows on the host,
// so nothing here is transcendental). One element: x0 from eps (or given), optional clamp, the order-1 terms, and the
// history term only where the row has one; every op is a separate rounding.
struct DpmRow {
  float sa, s1, cx, c0, c1;
};

DMC_DEV void dpm_elem(const DpmRow& r, bool from_eps, int clip, float x, float e, float x0, float xp, float& o,
                      float& x0o) {
  if (from_eps) {
    const float num = x - r.s1 * e;
    x0 = num / r.sa;
  }
  if (clip) x0 = fminf(fmaxf(x0, -1.0f), 1.0f);
  const float u = r.cx * x;
  const float v = r.c0 * x0;
  float y = u + v;
  if (r.c1 != 0.f) y = y + r.c1 * xp;
  o = y;
  x0o = x0;
}

// blockIdx.y strides over samples, blockIdx.x over the sample's elements: the row index and the five coefficients
// are block-uniform, read once per sample. VEC: 16-byte accesses (per % 4 == 0 and every pointer 16-byte aligned).
// x0_out may alias x0_prev: an element's history is read before the same thread writes that element.
template <bool VEC>
__global__ __launch_bounds__(256) void dpm_step_kernel(const float* x, const float* eps, const float* x0_in,
                                                       const float* x0_prev, const int64_t* step, const float* coef,
                                                       int S, int N, int per, int clip, float* out, float* x0_out) {
  const bool from_eps = x0_in == nullptr;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    long s = step[n];
    s = s < 0 ? 0 : (s > S - 1 ? S - 1 : s);   // never index past the table
    const float* c = coef + s * 5;
    const DpmRow r{c[0], c[1], c[2], c[3], c[4]};
    const bool hist = r.c1 != 0.f && x0_prev != nullptr;
    const float nohist = r.c1 != 0.f ? NAN : 0.f;   // an order-2 row without a history buffer: NaN out, no fault
    const size_t base = (size_t)n * per;
    if (VEC) {
      const int per4 = per / 4;
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per4; q += gridDim.x * blockDim.x) {
        const size_t i = base + (size_t)q * 4;
        const v4f xv = *(const v4f*)(x + i);
        v4f ev = {0.f, 0.f, 0.f, 0.f}, x0v = ev, pv = {nohist, nohist, nohist, nohist}, ov, x0ov;
        if (from_eps) ev = *(const v4f*)(eps + i);
        else x0v = *(const v4f*)(x0_in + i);
        if (hist) pv = *(const v4f*)(x0_prev + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float o, x0o;
          dpm_elem(r, from_eps, clip, xv[k], ev[k], x0v[k], pv[k], o, x0o);
          ov[k] = o;
          x0ov[k] = x0o;
        }
        *(v4f*)(out + i) = ov;
        *(v4f*)(x0_out + i) = x0ov;
      }
    } else {
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per; q += gridDim.x * blockDim.x) {
        const size_t i = base + q;
        float o, x0o;
        dpm_elem(r, from_eps, clip, x[i], from_eps ? eps[i] : 0.f, from_eps ? 0.f : x0_in[i],
                 hist ? x0_prev[i] : nohist, o, x0o);
        out[i] = o;
        x0_out[i] = x0o;
      }
    }
  }
}

// Known-region blend for editing samplers: inpainting as RePaint (Lugmayr et al. 2022, arXiv:2201.09865, algorithm 1:
// the known region is the given image noised to the step's target level, the rest the sampler's own output, and a
// resampling repetition jumps forward again) and the start of SDEdit's image-to-image (Meng et al. 2021,
// arXiv:2108.01073). diffusion/_edit.py builds the coefficient rows on the host, so nothing here is transcendental.
// One element: the noised known value, the blend, and the re-noise only where the row has one; every op is a separate
// rounding.
struct BlendRow {
  float ka, kb, ra, rb;
};

DMC_DEV float blend_elem(const BlendRow& r, float x, float x0, float m, float z, float z2) {
  float known = r.ka * x0;
  if (r.kb != 0.f) known = known + r.kb * z;
  const float u = m * known;
  const float w = (1.0f - m) * x;
  float b = u + w;
  if (r.rb != 0.f) {
    const float p = r.ra * b;
    b = p + r.rb * z2;
  }
  return b;
}

// Grid as dpm_step_kernel: blockIdx.y strides over samples, blockIdx.x over the sample's elements; the row index and
// its four coefficients are block-uniform, read once per sample. The mask holds mask_per values per sample, element j
// reads mask[n*mask_per + j % mask_per] (a per-pixel mask shared by the channels of NCHW). VEC: 16-byte accesses
// (per % 4 == 0, mask_per % 4 == 0, every pointer 16-byte aligned): four consecutive elements then sit in one mask
// period. out may alias x: an element is read before the same thread writes it.
template <bool VEC>
__global__ __launch_bounds__(256) void known_blend_kernel(const float* x, const float* x0, const float* mask,
                                                          int mask_per, const float* z, const float* z2,
                                                          const int64_t* row, const float* coef, int R, int N, int per,
                                                          float* out) {
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    long s = row[n];
    s = s < 0 ? 0 : (s > R - 1 ? R - 1 : s);   // never index past the table
    const float* c = coef + s * 4;
    const BlendRow r{c[0], c[1], c[2], c[3]};
    const bool rz = r.kb != 0.f && z != nullptr, rz2 = r.rb != 0.f && z2 != nullptr;
    const float noz = r.kb != 0.f ? NAN : 0.f;    // a noised row without its noise buffer: NaN out, no fault
    const float noz2 = r.rb != 0.f ? NAN : 0.f;
    const size_t base = (size_t)n * per;
    const float* mrow = mask + (size_t)n * mask_per;
    if (VEC) {
      const int per4 = per / 4;
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per4; q += gridDim.x * blockDim.x) {
        const size_t i = base + (size_t)q * 4;
        const v4f xv = *(const v4f*)(x + i);
        const v4f x0v = *(const v4f*)(x0 + i);
        const v4f mv = *(const v4f*)(mrow + (q * 4) % mask_per);
        v4f zv = {noz, noz, noz, noz}, z2v = {noz2, noz2, noz2, noz2}, ov;
        if (rz) zv = *(const v4f*)(z + i);
        if (rz2) z2v = *(const v4f*)(z2 + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) ov[k] = blend_elem(r, xv[k], x0v[k], mv[k], zv[k], z2v[k]);
        *(v4f*)(out + i) = ov;
      }
    } else {
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per; q += gridDim.x * blockDim.x) {
        const size_t i = base + q;
        out[i] = blend_elem(r, x[i], x0[i], mrow[q % mask_per], rz ? z[i] : noz, rz2 ? z2[i] : noz2);
      }
    }
  }
}

// The threshold tail of the two CFG kernels, by the whole block: sv holds |x0| of the row x0 (padding +inf), written
// by the caller without a barrier. p in (0,1): s = max(quantile_p |x0|, 1), x0 = clamp(x0, -s, s) / s; else clamp +-1.
DMC_DEV void cfg_threshold(float* sv, float* x0, int per, int npad, float p) {
  __syncthreads();
  if (!(p > 0.f)) {
    for (int i = threadIdx.x; i < per; i += blockDim.x) x0[i] = fminf(fmaxf(x0[i], -1.0f), 1.0f);
    return;
  }
  // bitonic sort of |x0| (padding +inf sorts last)
  for (int k = 2; k <= npad; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < npad; i += blockDim.x) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const float a = sv[i], b = sv[ixj];
          const bool up = (i & k) == 0;
          if ((a > b) == up) { sv[i] = b; sv[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }
  // torch.quantile(..., interpolation='linear'): rank = q*(n-1) in fp32, lerp
  const float rank = p * (float)(per - 1);
  const float lof = floorf(rank);
  const int lo = (int)lof;
  const int hi = (int)ceilf(rank);
  const float w = rank - lof;
  const float a = sv[lo], b = sv[hi];
  float s = (w < 0.5f) ? a + w * (b - a) : b - (b - a) * (1.0f - w);
  s = fmaxf(s, 1.0f);
  for (int i = threadIdx.x; i < per; i += blockDim.x) x0[i] = fminf(fmaxf(x0[i], -s), s) / s;
}

// One block per sample: CFG combine, x0 prediction, optional dynamic threshold (torch.quantile, linear).
__global__ __launch_bounds__(1024) void cfg_x0_kernel(const float* x, const float* ec, const float* eu, float scale,
                                                      const int64_t* t, const float* ta, const float* tb, int mode,
                                                      int per, int npad, float p, float* eps_out, float* x0_out) {
  extern __shared__ float sv[];
  const int n = blockIdx.x;
  const float* xr = x + (size_t)n * per;
  const long tt = t[n];
  for (int i = threadIdx.x; i < npad; i += blockDim.x) {
    float v = INFINITY;
    if (i < per) {
      float e;
      if (eu) {
        const float d = ec[(size_t)n * per + i] - eu[(size_t)n * per + i];
        e = eu[(size_t)n * per + i] + scale * d;
      } else {
        e = ec[(size_t)n * per + i];
      }
      if (eps_out) eps_out[(size_t)n * per + i] = e;
      float x0;
      if (mode == 0) {
        const float at = ta[tt];
        const float num = xr[i] - sqrtf(1.0f - at) * e;
        x0 = num / sqrtf(at);
      } else {
        const float u = ta[tt] * xr[i];
        const float w = tb[tt] * e;
        x0 = u - w;
      }
      x0_out[(size_t)n * per + i] = x0;
      v = fabsf(x0);
    }
    sv[i] = v;
  }
  cfg_threshold(sv, x0_out + (size_t)n * per, per, npad, p);
}

// Guided prediction, optional guidance rescale (Lin et al. 2023, arXiv:2305.08891 §3.4), eps and x0 from either
// prediction type, dynamic threshold; one block per sample, pc / pu rows read in place at their own strides. The v
// arm is pred_convert_kernel's ops (no division: alpha = 0 is representable). The rescale factor comes from two-pass
// double sums in a fixed order (thread-strided, wave butterfly, wave partials in index order): no atomics.
DMC_DEV void guide_block_sum2(double& a, double& b, double* sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    a += __shfl_xor(a, o, 64);
    b += __shfl_xor(b, o, 64);
  }
  const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    sm[2 * w] = a;
    sm[2 * w + 1] = b;
  }
  __syncthreads();
  a = 0.0;
  b = 0.0;
  for (int k = 0; k < nw; ++k) {
    a += sm[2 * k];
    b += sm[2 * k + 1];
  }
  __syncthreads();   // sm is reused
}

__global__ __launch_bounds__(1024) void cfg_guide_kernel(int pred_type, const float* x, const float* pc, long pc_ld,
                                                         const float* pu, long pu_ld, float scale, float rescale,
                                                         const int64_t* t, const float* sa, const float* s1, int T,
                                                         int per, int npad, float p, float* eps_out, float* x0_out) {
  extern __shared__ double guide_sm[];   // the wave partials of the sums, then |x0| for the sort (>= 256 bytes)
  float* sv = (float*)guide_sm;
  const int n = blockIdx.x;
  const float* xr = x + (size_t)n * per;
  const float* cr = pc + (size_t)n * pc_ld;
  const float* ur = pu + (size_t)n * pu_ld;
  const long tt = clamp_t(t[n], T);
  const float san = sa[tt], s1n = s1[tt];
  float f = 1.0f;
  if (rescale > 0.f) {
    double sc = 0.0, sg = 0.0;
    for (int i = threadIdx.x; i < per; i += blockDim.x) {
      const float c = cr[i], u = ur[i];
      const float d = c - u;
      const float g = u + scale * d;
      sc += (double)c;
      sg += (double)g;
    }
    guide_block_sum2(sc, sg, guide_sm);
    const double mc = sc / (double)per, mg = sg / (double)per;
    double qc = 0.0, qg = 0.0;
    for (int i = threadIdx.x; i < per; i += blockDim.x) {
      const float c = cr[i], u = ur[i];
      const float d = c - u;
      const float g = u + scale * d;
      const double dc = (double)c - mc, dg = (double)g - mg;
      qc += dc * dc;
      qg += dg * dg;
    }
    guide_block_sum2(qc, qg, guide_sm);
    // a guided row without spread has no deviation to match: it is left as it is (f = 1)
    if (qg > 0.0) f = (float)((double)rescale * sqrt(qc / qg) + (1.0 - (double)rescale));
  }
  for (int i = threadIdx.x; i < npad; i += blockDim.x) {
    float v = INFINITY;
    if (i < per) {
      const float c = cr[i], u = ur[i];
      const float d = c - u;
      float g = u + scale * d;
      if (rescale > 0.f) g = g * f;
      const float xx = xr[i];
      float e, x0;
      if (pred_type == DMC_PRED_V) {
        const float uu = s1n * xx;
        const float qq = san * g;
        e = uu + qq;
        const float pp = san * xx;
        const float rr = s1n * g;
        x0 = pp - rr;
      } else {
        e = g;
        const float num = xx - s1n * g;
        x0 = num / san;
      }
      if (eps_out) eps_out[(size_t)n * per + i] = e;
      x0_out[(size_t)n * per + i] = x0;
      v = fabsf(x0);
    }
    sv[i] = v;
  }
  cfg_threshold(sv, x0_out + (size_t)n * per, per, npad, p);
}

// Rectified-flow ODE step (Liu et al. 2022, arXiv:2209.03003; Heun as Karras et al. 2022, arXiv:2206.00364 alg. 1):
// guidance, Euler / Heun-predictor / Heun-corrector update and the history writes in one launch. diffusion/_flow.py
// builds the rows {sigma, h, hh, kind} on the host; nothing here is transcendental and every op is a separate rounding.
DMC_DEV float flow_velocity(float c, float u, bool guided, float scale) {
  if (!guided) return c;
  const float d = c - u;
  return u + scale * d;
}

// Grid as dpm_step_kernel: blockIdx.y strides over samples, blockIdx.x over the sample's elements; the row index, its
// step sizes and its kind are block-uniform, read once per sample. pc / pu rows sit at their own strides. VEC: 16-byte
// accesses (per, pc_ld and pu_ld multiples of 4, every pointer 16-byte aligned). out may alias x, xb_out xb and d_out
// dprev: an element is read before the same thread writes it.
template <bool VEC>
__global__ __launch_bounds__(256) void flow_step_kernel(const float* x, const float* pc, long pc_ld, const float* pu,
                                                        long pu_ld, float scale, const float* xb, const float* dprev,
                                                        const int64_t* step, const float* coef, int R, int N, int per,
                                                        float* out, float* xb_out, float* d_out) {
  const bool guided = pu != nullptr;
  for (int n = blockIdx.y; n < N; n += gridDim.y) {
    long s = step[n];
    s = s < 0 ? 0 : (s > R - 1 ? R - 1 : s);   // never index past the table
    const float* c = coef + s * 4;
    const float h = c[1], hh = c[2], kf = c[3];
    const int kind = kf == 1.f ? 1 : (kf == 2.f ? 2 : 0);
    const bool hist = kind == 2 && xb != nullptr && dprev != nullptr;   // a corrector row without history: NaN out
    const size_t base = (size_t)n * per;
    const float* cr = pc + (size_t)n * pc_ld;
    const float* ur = guided ? pu + (size_t)n * pu_ld : nullptr;
    if (VEC) {
      const int per4 = per / 4;
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per4; q += gridDim.x * blockDim.x) {
        const size_t i = base + (size_t)q * 4;
        const v4f cv = *(const v4f*)(cr + (size_t)q * 4);
        v4f uv = {0.f, 0.f, 0.f, 0.f}, gv, ov;
        if (guided) uv = *(const v4f*)(ur + (size_t)q * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) gv[k] = flow_velocity(cv[k], uv[k], guided, scale);
        if (kind == 2) {
          v4f bv = {NAN, NAN, NAN, NAN}, dv = bv;
          if (hist) {
            bv = *(const v4f*)(xb + i);
            dv = *(const v4f*)(dprev + i);
          }
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float sum = dv[k] + gv[k];
            ov[k] = bv[k] + hh * sum;
          }
        } else {
          const v4f xv = *(const v4f*)(x + i);
#pragma unroll
          for (int k = 0; k < 4; ++k) ov[k] = xv[k] + h * gv[k];
          if (kind == 1) {
            if (xb_out) *(v4f*)(xb_out + i) = xv;
            if (d_out) *(v4f*)(d_out + i) = gv;
          }
        }
        *(v4f*)(out + i) = ov;
      }
    } else {
      for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < per; q += gridDim.x * blockDim.x) {
        const size_t i = base + q;
        const float g = flow_velocity(cr[q], guided ? ur[q] : 0.f, guided, scale);
        float o;
        if (kind == 2) {
          const float b = hist ? xb[i] : NAN, d = hist ? dprev[i] : NAN;
          const float sum = d + g;
          o = b + hh * sum;
        } else {
          const float xx = x[i];
          o = xx + h * g;
          if (kind == 1) {
            if (xb_out) xb_out[i] = xx;
            if (d_out) d_out[i] = g;
          }
        }
        out[i] = o;
      }
    }
  }
}

// Guided velocity of a rectified flow with the guidance rescale and / or the dynamic threshold of cfg_guide_kernel: one
// block per sample, its launch shape, guide_block_sum2 and cfg_threshold unchanged. The threshold acts on the data
// prediction x0 = x - sigma*g (sigma from the sample's coefficient row); g_out holds x0 in between, so it must not
// alias x.
__global__ __launch_bounds__(1024) void flow_guide_kernel(const float* x, const float* pc, long pc_ld, const float* pu,
                                                          long pu_ld, float scale, float rescale, const int64_t* step,
                                                          const float* coef, int R, int per, int npad, int threshold,
                                                          float p, float* g_out) {
  extern __shared__ double guide_sm[];   // the wave partials of the sums, then |x0| for the sort (>= 256 bytes)
  float* sv = (float*)guide_sm;
  const int n = blockIdx.x;
  const float* cr = pc + (size_t)n * pc_ld;
  const float* ur = pu + (size_t)n * pu_ld;
  float* gr = g_out + (size_t)n * per;
  long s = step[n];
  s = s < 0 ? 0 : (s > R - 1 ? R - 1 : s);   // never index past the table
  const float sigma = coef[s * 4];
  float f = 1.0f;
  if (rescale > 0.f) {
    double sc = 0.0, sg = 0.0;
    for (int i = threadIdx.x; i < per; i += blockDim.x) {
      const float c = cr[i], u = ur[i];
      const float d = c - u;
      const float g = u + scale * d;
      sc += (double)c;
      sg += (double)g;
    }
    guide_block_sum2(sc, sg, guide_sm);
    const double mc = sc / (double)per, mg = sg / (double)per;
    double qc = 0.0, qg = 0.0;
    for (int i = threadIdx.x; i < per; i += blockDim.x) {
      const float c = cr[i], u = ur[i];
      const float d = c - u;
      const float g = u + scale * d;
      const double dc = (double)c - mc, dg = (double)g - mg;
      qc += dc * dc;
      qg += dg * dg;
    }
    guide_block_sum2(qc, qg, guide_sm);
    // a guided row without spread has no deviation to match: it is left as it is (f = 1)
    if (qg > 0.0) f = (float)((double)rescale * sqrt(qc / qg) + (1.0 - (double)rescale));
  }
  if (!threshold) {   // block-uniform
    for (int i = threadIdx.x; i < per; i += blockDim.x) {
      const float c = cr[i], u = ur[i];
      const float d = c - u;
      float g = u + scale * d;
      if (rescale > 0.f) g = g * f;
      gr[i] = g;
    }
    return;
  }
  const float* xr = x + (size_t)n * per;
  for (int i = threadIdx.x; i < npad; i += blockDim.x) {
    float v = INFINITY;
    if (i < per) {
      const float c = cr[i], u = ur[i];
      const float d = c - u;
      float g = u + scale * d;
      if (rescale > 0.f) g = g * f;
      const float w = sigma * g;
      const float x0 = xr[i] - w;
      gr[i] = x0;
      v = fabsf(x0);
    }
    sv[i] = v;
  }
  cfg_threshold(sv, gr, per, npad, p);
  // cfg_threshold's last pass gave element i to thread i % blockDim.x, as this one does: no barrier in between
  for (int i = threadIdx.x; i < per; i += blockDim.x) {
    const float num = xr[i] - gr[i];
    gr[i] = num / sigma;
  }
}

// ---------------- multi-tensor ----------------
__global__ void ema_kernel(const dmc_tensor_ref* refs, float decay) {
  const dmc_tensor_ref r = refs[blockIdx.y];
  const float om = 1.0f - decay;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < r.n; i += (long)gridDim.x * blockDim.x) {
    const float e = r.a[i] * decay;
    r.a[i] = e + om * r.b[i];
  }
}

constexpr int kClipSlices = 16;
__global__ __launch_bounds__(256) void sumsq_kernel(const dmc_tensor_ref* refs, float* partial) {
  const dmc_tensor_ref r = refs[blockIdx.y];
  float s = 0.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < r.n; i += (long)gridDim.x * blockDim.x) {
    const float g = r.a[i];
    s = fmaf(g, g, s);
  }
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.y * kClipSlices + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ void clip_coef_kernel(const float* partial, int count, float max_norm, float* total_norm, float* coef) {
  // norm of per-tensor norms (torch.nn.utils.clip_grad_norm_ structure), fixed order
  __shared__ float red[4];
  float s = 0.f;
  for (int t = threadIdx.x; t < count; t += blockDim.x) {
    float q = 0.f;
    for (int k = 0; k < kClipSlices; ++k) q += partial[t * kClipSlices + k];
    const float nt = sqrtf(q);
    s = fmaf(nt, nt, s);
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float tot = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
    total_norm[0] = tot;
    const float c = max_norm / (tot + 1e-6f);
    coef[0] = c < 1.0f ? c : 1.0f;
  }
}

__global__ void scale_kernel(const dmc_tensor_ref* refs, const float* coef) {
  const dmc_tensor_ref r = refs[blockIdx.y];
  const float c = coef[0];
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < r.n; i += (long)gridDim.x * blockDim.x) r.a[i] *= c;
}

// ---------------- flat optimizer step ----------------
// Parameters, gradients, AdamW moments and the EMA copy live in flat fp32 buffers with one common layout
// (the executor's gradient order), so clip + AdamW + EMA are one streaming pass over 37 M elements.
constexpr int kNormBlocks = 1024;   // 4096 measured no faster (34 us: the walk reads ~4.4 TB/s either way)
__global__ __launch_bounds__(256) void flat_sumsq_kernel(const float* g, long n, float* partial) {
  // block b sums the contiguous range [b*per, (b+1)*per): fixed order, deterministic
  const long per = ((n + kNormBlocks - 1) / kNormBlocks + 3) & ~3L;
  const long b0 = blockIdx.x * per, b1 = b0 + per < n ? b0 + per : n;
  // four 16-byte loads in flight per thread (one at a time left the walk latency-bound: 35 us for 148 MB),
  // four accumulators combined in a fixed order
  float s = 0.f, sa[4] = {0.f, 0.f, 0.f, 0.f};
  long i = b0 + threadIdx.x * 4;
  for (; i + 3 * 1024 + 3 < b1; i += 4 * 1024) {
    v4f v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *(const v4f*)(g + i + u * 1024);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      sa[u] = fmaf(v[u][0], v[u][0], sa[u]); sa[u] = fmaf(v[u][1], v[u][1], sa[u]);
      sa[u] = fmaf(v[u][2], v[u][2], sa[u]); sa[u] = fmaf(v[u][3], v[u][3], sa[u]);
    }
  }
  for (; i + 3 < b1; i += 1024) {
    const v4f v = *(const v4f*)(g + i);
    s = fmaf(v[0], v[0], s); s = fmaf(v[1], v[1], s); s = fmaf(v[2], v[2], s); s = fmaf(v[3], v[3], s);
  }
  for (; i < b1; ++i) s = fmaf(g[i], g[i], s);
  s += (sa[0] + sa[1]) + (sa[2] + sa[3]);
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void flat_norm_final(const float* partial, float max_norm, float* total_norm,
                                                       float* coef) {
  float s = 0.f;
  for (int k = threadIdx.x; k < kNormBlocks; k += 256) s += partial[k];
  __shared__ float red[4];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float tot = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
    total_norm[0] = tot;
    const float c = max_norm / (tot + 1e-6f);
    coef[0] = max_norm > 0.f ? (c < 1.0f ? c : 1.0f) : 1.0f;
  }
}

// torch.optim.AdamW (foreach, non-amsgrad) per element, in torch's operation order:
//   g *= clip;  p *= 1 - lr*wd;  m = lerp(m, g, 1-b1);  v = v*b2 + (1-b2)*g*g;
//   p += -step_size * m / (sqrt(v)/bc2_sqrt + eps);  then ema = ema*d + (1-d)*p  (utils/trainer.py:198-202)
struct AdamWArgs {
  float* p; const float* g; float* m; float* v; float* ema;
  const float* coef;
  long n;
  float wd_mul, w1, b2, omb2, neg_step, bc2_sqrt, eps, ema_d, ema_om;   // host-computed like torch (double -> float)
  const float* hyper;   // if set, the nine scalars are read from device memory (dmc_adamw_flat_dev order)
};

// the scalars of a graph-replayed step live in device memory, refreshed by one H2D copy per step
DMC_DEV AdamWArgs adamw_resolve(const AdamWArgs& a0) {
  AdamWArgs a = a0;
  if (const float* h = a0.hyper) {
    a.wd_mul = h[0]; a.w1 = h[1]; a.b2 = h[2]; a.omb2 = h[3]; a.eps = h[4];
    a.neg_step = h[5]; a.bc2_sqrt = h[6]; a.ema_d = h[7]; a.ema_om = h[8];
  }
  return a;
}

DMC_DEV void adamw_elem(const AdamWArgs& a, float c, float& p, float g, float& m, float& v, float* e) {
  g = g * c;
  p = p * a.wd_mul;
  m = (a.w1 < 0.5f) ? m + a.w1 * (g - m) : g - (g - m) * (1.0f - a.w1);
  v = v * a.b2;
  v = v + a.omb2 * (g * g);
  const float den = sqrtf(v) / a.bc2_sqrt + a.eps;
  p = p + a.neg_step * (m / den);
  if (e) *e = *e * a.ema_d + a.ema_om * p;
}

__global__ __launch_bounds__(256) void adamw_flat_kernel(AdamWArgs a0) {
  const AdamWArgs a = adamw_resolve(a0);
  const float c = a.coef ? a.coef[0] : 1.0f;
  const long n4 = a.n / 4;
  for (long q = blockIdx.x * (long)blockDim.x + threadIdx.x; q < n4; q += (long)gridDim.x * blockDim.x) {
    const long i = q * 4;
    v4f p = *(v4f*)(a.p + i), m = *(v4f*)(a.m + i), v = *(v4f*)(a.v + i);
    const v4f g = *(const v4f*)(a.g + i);
    v4f e;
    if (a.ema) e = *(v4f*)(a.ema + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float pk = p[k], mk = m[k], vk = v[k], ek = e[k];
      adamw_elem(a, c, pk, g[k], mk, vk, a.ema ? &ek : nullptr);
      p[k] = pk; m[k] = mk; v[k] = vk; e[k] = ek;
    }
    *(v4f*)(a.p + i) = p; *(v4f*)(a.m + i) = m; *(v4f*)(a.v + i) = v;
    if (a.ema) *(v4f*)(a.ema + i) = e;
  }
  // ragged tail (n % 4) handled by the first threads of block 0
  if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) {
    const long i = n4 * 4 + threadIdx.x;
    adamw_elem(a, c, a.p[i], a.g[i], a.m[i], a.v[i], a.ema ? a.ema + i : nullptr);
  }
}

template <typename T>
__global__ void unpack_kernel(const T* src, int ld, int N, int C, int H, int W, float* dst) {
  const long total = (long)N * C * H * W;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int hw = i % (H * W);
    const long r = i / (H * W);
    const int c = r % C;
    const int n = r / C;
    const size_t s = ((size_t)n * H * W + hw) * ld + c;
    dst[i] = sizeof(T) == 4 ? ((const float*)src)[s] : bf2f(((const bf16_t*)src)[s]);
  }
}

template <typename T>
__global__ void add_kernel(T* y, const T* x, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    if (sizeof(T) == 4) ((float*)y)[i] = ((const float*)y)[i] + ((const float*)x)[i];
    else ((bf16_t*)y)[i] = (bf16_t)f2bf(bf2f(((const bf16_t*)y)[i]) + bf2f(((const bf16_t*)x)[i]));
  }
}

// Nearest x2 upsample of an NHWC activation (models/unet.py:118 F.interpolate(scale_factor=2, mode='nearest')),
// materialised for the halo weight-gradient kernel: one 16-byte chunk read, four written per thread.
__global__ __launch_bounds__(256) void upsample2x_nhwc_kernel(const char* x, int N, int H, int W, int cb, int ldb,
                                                              char* y, int ldyb) {
  const int chunks = cb / 16;
  const long total = (long)N * H * W * chunks;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i % chunks);
    const long pix = i / chunks;
    const int w = (int)(pix % W);
    const long nh = pix / W;
    const int h = (int)(nh % H), n = (int)(nh / H);
    const v4i v = *(const v4i*)(x + pix * ldb + ch * 16);
    const long o = (((long)n * 2 * H + 2 * h) * 2 * W + 2 * w) * ldyb + ch * 16;
    *(v4i*)(y + o) = v;
    *(v4i*)(y + o + ldyb) = v;
    *(v4i*)(y + o + (long)2 * W * ldyb) = v;
    *(v4i*)(y + o + (long)2 * W * ldyb + ldyb) = v;
  }
}

__global__ void silu_kernel(const float* x, float* y, long n) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float v = x[i];
    y[i] = v / (1.0f + expf(-v));
  }
}

}  // namespace

extern "C" int dmc_time_embed(const int64_t* t, int B, int dim, float* out, void* stream) {
  DMC_REQUIRE(dim % 2 == 0 && dim >= 4, "time_embed: dim %d", dim);
  time_embed_kernel<<<grid_for((long)B * dim / 2), 256, 0, dmc::as_stream(stream)>>>(t, B, dim, out);
  return dmc::check_launch("dmc_time_embed");
}

extern "C" int dmc_embed_fwd(const int64_t* y, int B, int rows, const float* table, int dim, float* out, void* stream) {
  embed_fwd_kernel<<<grid_for((long)B * dim), 256, 0, dmc::as_stream(stream)>>>(y, B, rows, table, dim, out);
  return dmc::check_launch("dmc_embed_fwd");
}

extern "C" int dmc_embed_bwd(const int64_t* y, int B, int rows, const float* dout, int dim, float* dtable, void* stream) {
  embed_bwd_kernel<<<grid_for((long)rows * dim), 256, 0, dmc::as_stream(stream)>>>(y, B, rows, dout, dim, dtable);
  return dmc::check_launch("dmc_embed_bwd");
}

extern "C" int dmc_pack_input(int dtype, const float* x, const float* noise, const int64_t* t, const float* a,
                              const float* b, int N, int C, int H, int W, void* dst, int ld, void* stream) {
  DMC_REQUIRE(ld >= C, "pack_input: ld %d < C %d", ld, C);
  const long total = (long)N * H * W * ld;
  hipStream_t s = dmc::as_stream(stream);
  if (dtype == DMC_F32)
    pack_input_kernel<float><<<grid_for(total), 256, 0, s>>>(x, noise, t, a, b, N, C, H, W, (float*)dst, ld);
  else
    pack_input_kernel<bf16_t><<<grid_for(total), 256, 0, s>>>(x, noise, t, a, b, N, C, H, W, (bf16_t*)dst, ld);
  return dmc::check_launch("dmc_pack_input");
}

extern "C" int dmc_q_sample(const float* x0, const float* noise, const int64_t* t, const float* a, const float* b, int N,
                            int per, float* out, void* stream) {
  const long total = (long)N * per;
  q_sample_kernel<<<grid_for(total), 256, 0, dmc::as_stream(stream)>>>(x0, noise, t, a, b, total, per, out);
  return dmc::check_launch("dmc_q_sample");
}

extern "C" int dmc_loss_fwd(int type, const float* pred, const float* target, long n, float* loss, float* ws,
                            void* stream) {
  DMC_REQUIRE(type >= 0 && type <= 2, "loss: type %d", type);
  hipStream_t s = dmc::as_stream(stream);
  const int nb = grid_for(n, 256, 1024);
  loss_partial_kernel<<<nb, 256, 0, s>>>(type, pred, target, n, ws);
  loss_final_kernel<<<1, 256, 0, s>>>(ws, nb, n, loss);
  return dmc::check_launch("dmc_loss_fwd");
}

extern "C" int dmc_loss_bwd(int type, const float* pred, const float* target, long n, const float* dloss, float* dpred,
                            void* stream) {
  DMC_REQUIRE(type >= 0 && type <= 2, "loss: type %d", type);
  loss_bwd_kernel<<<grid_for(n), 256, 0, dmc::as_stream(stream)>>>(type, pred, target, n, dloss, dpred);
  return dmc::check_launch("dmc_loss_bwd");
}

namespace {
// (gx, gy) of the sample-per-blockIdx.y kernels: at most xcap blocks along a sample, at most 16384 blocks in all
inline dim3 sample_grid(int units, int N, int xcap) {
  const int gx = grid_for(units, 256, xcap);
  const int gy_cap = 16384 / gx > 0 ? 16384 / gx : 1;
  return dim3(gx, N < gy_cap ? N : gy_cap);
}
}  // namespace

// dmc_objective and dmc_objective_is: the same two kernels, iw and row_loss NULL for the former
static int objective_launch(const char* what, int pred_type, int type, const float* pred, const float* x0,
                            const float* noise, const int64_t* t, const float* sa, const float* s1, const float* w,
                            const float* iw, int T, int N, int per, const float* dloss, float* loss, float* row_loss,
                            float* dpred, float* ws, void* stream) {
  DMC_REQUIRE(pred_type == DMC_PRED_EPS || pred_type == DMC_PRED_V, "objective: prediction type %d", pred_type);
  DMC_REQUIRE(type >= 0 && type <= 2, "objective: loss type %d", type);
  DMC_REQUIRE(T > 0 && N > 0 && per > 0, "objective: T %d, N %d, per_sample %d must be positive", T, N, per);
  DMC_REQUIRE(pred && noise && t && loss && ws, "objective: pred, noise, t, loss and workspace must not be NULL");
  DMC_REQUIRE(pred_type == DMC_PRED_EPS || (x0 && sa && s1), "objective: v-prediction needs x0 and both tables");
  DMC_REQUIRE(!dpred || dloss, "objective: dpred needs the upstream gradient dloss");
  const uintptr_t bits = (uintptr_t)pred | (uintptr_t)noise | (uintptr_t)dpred |
                         (pred_type == DMC_PRED_V ? (uintptr_t)x0 : 0);   // a NULL or unread operand adds no bits
  const bool vec = per % 4 == 0 && (bits & 15) == 0;
  const dim3 grid = sample_grid(vec ? per / 4 : per, N, DMC_OBJECTIVE_MAX_BLOCKS);
  hipStream_t s = dmc::as_stream(stream);
#define DMC_OBJECTIVE_LAUNCH(VEC, IS)                                                                                 \
  objective_kernel<VEC, IS><<<grid, 256, 0, s>>>(pred_type, type, pred, x0, noise, t, sa, s1, w, iw, T, N, per, dloss, \
                                                 dpred, ws)
  if (vec && iw) DMC_OBJECTIVE_LAUNCH(true, true);
  else if (vec) DMC_OBJECTIVE_LAUNCH(true, false);
  else if (iw) DMC_OBJECTIVE_LAUNCH(false, true);
  else DMC_OBJECTIVE_LAUNCH(false, false);
#undef DMC_OBJECTIVE_LAUNCH
  objective_final_kernel<<<1, 256, 0, s>>>(ws, (int)grid.x, t, w, iw, T, N, per, loss, row_loss);
  return dmc::check_launch(what);
}

extern "C" int dmc_objective(int pred_type, int type, const float* pred, const float* x0, const float* noise,
                             const int64_t* t, const float* sa, const float* s1, const float* w, int T, int N, int per,
                             const float* dloss, float* loss, float* dpred, float* ws, void* stream) {
  return objective_launch("dmc_objective", pred_type, type, pred, x0, noise, t, sa, s1, w, nullptr, T, N, per, dloss,
                          loss, nullptr, dpred, ws, stream);
}

extern "C" int dmc_objective_is(int pred_type, int type, const float* pred, const float* x0, const float* noise,
                                const int64_t* t, const float* sa, const float* s1, const float* w, const float* iw,
                                int T, int N, int per, const float* dloss, float* loss, float* row_loss, float* dpred,
                                float* ws, void* stream) {
  return objective_launch("dmc_objective_is", pred_type, type, pred, x0, noise, t, sa, s1, w, iw, T, N, per, dloss,
                          loss, row_loss, dpred, ws, stream);
}

extern "C" int dmc_pred_convert(int pred_type, const float* x, const int64_t* t, const float* sa, const float* s1,
                                int T, const float* pred, int reps, int N, int per, float* eps_out, float* x0_out,
                                void* stream) {
  DMC_REQUIRE(pred_type == DMC_PRED_V, "pred_convert: prediction type %d (eps needs no conversion)", pred_type);
  DMC_REQUIRE(T > 0 && N > 0 && per > 0 && reps > 0,
              "pred_convert: T %d, N %d, per_sample %d, reps %d must be positive", T, N, per, reps);
  DMC_REQUIRE(x && t && sa && s1 && pred && eps_out, "pred_convert: only x0_out may be NULL");
  const uintptr_t bits = (uintptr_t)x | (uintptr_t)pred | (uintptr_t)eps_out | (uintptr_t)x0_out;
  const bool vec = per % 4 == 0 && (bits & 15) == 0;
  const dim3 grid = sample_grid(vec ? per / 4 : per, N, 8192);
  hipStream_t s = dmc::as_stream(stream);
  if (vec) pred_convert_kernel<true><<<grid, 256, 0, s>>>(x, t, sa, s1, T, pred, reps, N, per, eps_out, x0_out);
  else pred_convert_kernel<false><<<grid, 256, 0, s>>>(x, t, sa, s1, T, pred, reps, N, per, eps_out, x0_out);
  return dmc::check_launch("dmc_pred_convert");
}

extern "C" int dmc_vlb_step(const float* x0, const float* x_t, const float* pred, const int64_t* t, const float* coef,
                            int T, int clip, const float* z_next, const int64_t* t_next, const float* sa, const float* s1,
                            int N, int per, float* x_next, float* vb, float* xstart_mse, float* eps_mse, float* x0_sq,
                            float* ws, void* stream) {
  DMC_REQUIRE(T > 0 && N > 0 && per > 0, "vlb_step: T %d, N %d, per_sample %d must be positive", T, N, per);
  DMC_REQUIRE(x0 && x_t && pred && t && coef && vb && xstart_mse && eps_mse && x0_sq && ws,
              "vlb_step: only x_next and its operands z_next, t_next, sa, s1 may be NULL");
  DMC_REQUIRE(!x_next || (z_next && t_next && sa && s1), "vlb_step: x_next needs z_next, t_next and both tables");
  const uintptr_t bits = (uintptr_t)x0 | (uintptr_t)x_t | (uintptr_t)pred | (uintptr_t)x_next |
                         (x_next ? (uintptr_t)z_next : 0);   // a NULL or unread operand adds no bits
  const bool vec = per % 4 == 0 && (bits & 15) == 0;
  const dim3 grid = sample_grid(vec ? per / 4 : per, N, DMC_VLB_MAX_BLOCKS);
  hipStream_t s = dmc::as_stream(stream);
  if (vec)
    vlb_step_kernel<true><<<grid, 256, 0, s>>>(x0, x_t, pred, t, coef, T, clip, z_next, t_next, sa, s1, N, per, x_next, ws);
  else
    vlb_step_kernel<false><<<grid, 256, 0, s>>>(x0, x_t, pred, t, coef, T, clip, z_next, t_next, sa, s1, N, per, x_next,
                                                ws);
  vlb_final_kernel<<<(N + 255) / 256, 256, 0, s>>>(ws, (int)grid.x, t, coef, 6, 4, T, N, per, vb, xstart_mse, eps_mse,
                                                   x0_sq);
  return dmc::check_launch("dmc_vlb_step");
}

// dmc_hybrid_objective and dmc_hybrid_objective_is, as objective_launch
static int hybrid_launch(const char* what, int pred_type, int type, const float* out, const float* x0,
                         const float* noise, const int64_t* t, const float* sa, const float* s1, const float* w,
                         const float* iw, const float* coef, int T, int N, int per, float vlb_weight,
                         const float* dloss, float* loss, float* row_loss, float* dout, float* ws, void* stream) {
  DMC_REQUIRE(pred_type == DMC_PRED_EPS || pred_type == DMC_PRED_V, "hybrid_objective: prediction type %d", pred_type);
  DMC_REQUIRE(type >= 0 && type <= 2, "hybrid_objective: loss type %d", type);
  DMC_REQUIRE(T > 0 && N > 0 && per > 0, "hybrid_objective: T %d, N %d, per_sample %d must be positive", T, N, per);
  DMC_REQUIRE(out && x0 && noise && t && coef && loss && ws,
              "hybrid_objective: out, x0, noise, t, coef, loss and workspace must not be NULL");
  DMC_REQUIRE(pred_type == DMC_PRED_EPS || (sa && s1), "hybrid_objective: v-prediction needs both tables");
  DMC_REQUIRE(!dout || dloss, "hybrid_objective: dout needs the upstream gradient dloss");
  const uintptr_t bits = (uintptr_t)out | (uintptr_t)x0 | (uintptr_t)noise | (uintptr_t)dout;
  const bool vec = per % 4 == 0 && (bits & 15) == 0;   // then the v halves, per floats further on, are aligned too
  const dim3 grid = sample_grid(vec ? per / 4 : per, N, DMC_OBJECTIVE_MAX_BLOCKS);
  hipStream_t s = dmc::as_stream(stream);
#define DMC_HYBRID_LAUNCH(VEC, GRAD)                                                                                  \
  do {                                                                                                                \
    if (iw && GRAD)   /* the forward alone never reads iw */                                                          \
      hybrid_objective_kernel<VEC, GRAD, true><<<grid, 256, 0, s>>>(pred_type, type, out, x0, noise, t, sa, s1, w, iw, \
                                                                    coef, T, N, per, vlb_weight, dloss, dout, ws);    \
    else                                                                                                              \
      hybrid_objective_kernel<VEC, GRAD, false><<<grid, 256, 0, s>>>(pred_type, type, out, x0, noise, t, sa, s1, w,   \
                                                                     iw, coef, T, N, per, vlb_weight, dloss, dout, ws); \
  } while (0)
  if (vec && dout) DMC_HYBRID_LAUNCH(true, true);
  else if (vec) DMC_HYBRID_LAUNCH(true, false);
  else if (dout) DMC_HYBRID_LAUNCH(false, true);
  else DMC_HYBRID_LAUNCH(false, false);
#undef DMC_HYBRID_LAUNCH
  hybrid_final_kernel<<<1, 256, 0, s>>>(ws, (int)grid.x, t, w, iw, T, N, per, vlb_weight, loss, row_loss);
  return dmc::check_launch(what);
}

extern "C" int dmc_hybrid_objective(int pred_type, int type, const float* out, const float* x0, const float* noise,
                                    const int64_t* t, const float* sa, const float* s1, const float* w,
                                    const float* coef, int T, int N, int per, float vlb_weight, const float* dloss,
                                    float* loss, float* dout, float* ws, void* stream) {
  return hybrid_launch("dmc_hybrid_objective", pred_type, type, out, x0, noise, t, sa, s1, w, nullptr, coef, T, N, per,
                       vlb_weight, dloss, loss, nullptr, dout, ws, stream);
}

extern "C" int dmc_hybrid_objective_is(int pred_type, int type, const float* out, const float* x0, const float* noise,
                                       const int64_t* t, const float* sa, const float* s1, const float* w,
                                       const float* iw, const float* coef, int T, int N, int per, float vlb_weight,
                                       const float* dloss, float* loss, float* row_loss, float* dout, float* ws,
                                       void* stream) {
  return hybrid_launch("dmc_hybrid_objective_is", pred_type, type, out, x0, noise, t, sa, s1, w, iw, coef, T, N, per,
                       vlb_weight, dloss, loss, row_loss, dout, ws, stream);
}

extern "C" int dmc_vlb_step_learned(const float* x0, const float* x_t, const float* pred, long pred_stride,
                                    const float* v, long v_stride, const int64_t* t, const float* coef, int T,
                                    int clip, const float* z_next, const int64_t* t_next, const float* sa,
                                    const float* s1, int N, int per, float* x_next, float* vb, float* xstart_mse,
                                    float* eps_mse, float* x0_sq, float* ws, void* stream) {
  DMC_REQUIRE(T > 0 && N > 0 && per > 0, "vlb_step_learned: T %d, N %d, per_sample %d must be positive", T, N, per);
  DMC_REQUIRE(x0 && x_t && pred && v && t && coef && vb && xstart_mse && eps_mse && x0_sq && ws,
              "vlb_step_learned: only x_next and its operands z_next, t_next, sa, s1 may be NULL");
  DMC_REQUIRE(pred_stride >= per && v_stride >= per, "vlb_step_learned: row strides %ld, %ld below per_sample %d",
              pred_stride, v_stride, per);
  DMC_REQUIRE(!x_next || (z_next && t_next && sa && s1),
              "vlb_step_learned: x_next needs z_next, t_next and both tables");
  const uintptr_t bits = (uintptr_t)x0 | (uintptr_t)x_t | (uintptr_t)pred | (uintptr_t)v | (uintptr_t)x_next |
                         (x_next ? (uintptr_t)z_next : 0);   // a NULL or unread operand adds no bits
  const bool vec = per % 4 == 0 && pred_stride % 4 == 0 && v_stride % 4 == 0 && (bits & 15) == 0;
  const dim3 grid = sample_grid(vec ? per / 4 : per, N, DMC_VLB_MAX_BLOCKS);
  hipStream_t s = dmc::as_stream(stream);
  if (vec)
    vlb_step_learned_kernel<true><<<grid, 256, 0, s>>>(x0, x_t, pred, pred_stride, v, v_stride, t, coef, T, clip, z_next,
                                                       t_next, sa, s1, N, per, x_next, ws);
  else
    vlb_step_learned_kernel<false><<<grid, 256, 0, s>>>(x0, x_t, pred, pred_stride, v, v_stride, t, coef, T, clip,
                                                        z_next, t_next, sa, s1, N, per, x_next, ws);
  vlb_final_kernel<<<(N + 255) / 256, 256, 0, s>>>(ws, (int)grid.x, t, coef, DMC_LVAR_COLS, 6, T, N, per, vb,
                                                   xstart_mse, eps_mse, x0_sq);
  return dmc::check_launch("dmc_vlb_step_learned");
}

extern "C" int dmc_ddpm_step_learned(const float* x, const float* eps, long eps_stride, const float* v, long v_stride,
                                     const float* x0_in, const int64_t* t, const float* sra, const float* srm1,
                                     const float* c1, const float* c2, const float* coef, int T, int N, int per,
                                     int clip, const float* z, float* out, void* stream) {
  DMC_REQUIRE(T > 0 && N > 0 && per > 0, "ddpm_step_learned: T %d, N %d, per_sample %d must be positive", T, N, per);
  DMC_REQUIRE(x && (eps || x0_in) && t && c1 && c2 && coef && out,
              "ddpm_step_learned: x, eps (or x0_in), t, the tables and out must not be NULL");
  DMC_REQUIRE(x0_in || (sra && srm1), "ddpm_step_learned: an eps input needs the sqrt_recip tables");
  DMC_REQUIRE(!z || v, "ddpm_step_learned: z needs v");
  DMC_REQUIRE((x0_in || eps_stride >= per) && (!z || v_stride >= per),
              "ddpm_step_learned: row strides %ld, %ld below per_sample %d", eps_stride, v_stride, per);
  const bool rd_eps = x0_in == nullptr, rd_v = z != nullptr;
  const uintptr_t bits = (uintptr_t)x | (uintptr_t)out | (uintptr_t)x0_in | (uintptr_t)z |
                         (rd_eps ? (uintptr_t)eps : 0) | (rd_v ? (uintptr_t)v : 0);   // unread operands add no bits
  const bool vec = per % 4 == 0 && (bits & 15) == 0 && (!rd_eps || eps_stride % 4 == 0) &&
                   (!rd_v || v_stride % 4 == 0);
  const dim3 grid = sample_grid(vec ? per / 4 : per, N, 8192);
  hipStream_t s = dmc::as_stream(stream);
  if (vec)
    ddpm_step_learned_kernel<true><<<grid, 256, 0, s>>>(x, eps, eps_stride, v, v_stride, x0_in, t, sra, srm1, c1, c2,
                                                        coef, T, N, per, clip, z, out);
  else
    ddpm_step_learned_kernel<false><<<grid, 256, 0, s>>>(x, eps, eps_stride, v, v_stride, x0_in, t, sra, srm1, c1, c2,
                                                         coef, T, N, per, clip, z, out);
  return dmc::check_launch("dmc_ddpm_step_learned");
}

extern "C" int dmc_ddim_step(const float* x, const float* eps, const float* x0_in, const int64_t* t, const int64_t* t_next,
                             const float* ac, int N, int per, float eta, int clip, const float* z, float* out,
                             void* stream) {
  ddim_step_kernel<<<grid_for((long)N * per), 256, 0, dmc::as_stream(stream)>>>(x, eps, x0_in, t, t_next, ac, N, per, eta,
                                                                                 clip, z, out);
  return dmc::check_launch("dmc_ddim_step");
}

extern "C" int dmc_ddpm_step(const float* x, const float* eps, const float* x0_in, const int64_t* t, const float* sra,
                             const float* srm1, const float* c1, const float* c2, const float* lv, int N, int per,
                             int clip, const float* z, float* out, void* stream) {
  ddpm_step_kernel<<<grid_for((long)N * per), 256, 0, dmc::as_stream(stream)>>>(x, eps, x0_in, t, sra, srm1, c1, c2, lv,
                                                                                 N, per, clip, z, out);
  return dmc::check_launch("dmc_ddpm_step");
}

extern "C" int dmc_dpm_step(const float* x, const float* eps, const float* x0_in, const float* x0_prev,
                            const int64_t* step, const float* coef, int S, int N, int per, int clip, float* out,
                            float* x0_out, void* stream) {
  DMC_REQUIRE(S > 0 && N > 0 && per > 0, "dpm_step: S %d, N %d, per_sample %d must be positive", S, N, per);
  DMC_REQUIRE(x && step && coef && out && x0_out, "dpm_step: x, step, coef, out and x0_out must not be NULL");
  DMC_REQUIRE(eps || x0_in, "dpm_step: eps may be NULL only when x0_in is given");
  const uintptr_t bits = (uintptr_t)x | (uintptr_t)eps | (uintptr_t)x0_in | (uintptr_t)x0_prev | (uintptr_t)out |
                         (uintptr_t)x0_out;   // a NULL operand adds no bits
  const bool vec = per % 4 == 0 && (bits & 15) == 0;
  const int gx = grid_for(vec ? per / 4 : per);
  const int gy_cap = 16384 / gx > 0 ? 16384 / gx : 1;
  const dim3 grid(gx, N < gy_cap ? N : gy_cap);
  hipStream_t s = dmc::as_stream(stream);
  if (vec) dpm_step_kernel<true><<<grid, 256, 0, s>>>(x, eps, x0_in, x0_prev, step, coef, S, N, per, clip, out, x0_out);
  else dpm_step_kernel<false><<<grid, 256, 0, s>>>(x, eps, x0_in, x0_prev, step, coef, S, N, per, clip, out, x0_out);
  return dmc::check_launch("dmc_dpm_step");
}

extern "C" int dmc_known_blend(const float* x, const float* x0, const float* mask, int mask_per, const float* z,
                               const float* z2, const int64_t* row, const float* coef, int R, int N, int per,
                               float* out, void* stream) {
  DMC_REQUIRE(R > 0 && N > 0 && per > 0 && mask_per > 0,
              "known_blend: R %d, N %d, per_sample %d, mask_per %d must be positive", R, N, per, mask_per);
  DMC_REQUIRE(per % mask_per == 0, "known_blend: mask_per %d does not divide per_sample %d", mask_per, per);
  DMC_REQUIRE(x && x0 && mask && row && coef && out, "known_blend: only z and z2 may be NULL");
  const uintptr_t bits = (uintptr_t)x | (uintptr_t)x0 | (uintptr_t)mask | (uintptr_t)z | (uintptr_t)z2 |
                         (uintptr_t)out;   // a NULL operand adds no bits
  const bool vec = per % 4 == 0 && mask_per % 4 == 0 && (bits & 15) == 0;
  const dim3 grid = sample_grid(vec ? per / 4 : per, N, 8192);
  hipStream_t s = dmc::as_stream(stream);
  if (vec) known_blend_kernel<true><<<grid, 256, 0, s>>>(x, x0, mask, mask_per, z, z2, row, coef, R, N, per, out);
  else known_blend_kernel<false><<<grid, 256, 0, s>>>(x, x0, mask, mask_per, z, z2, row, coef, R, N, per, out);
  return dmc::check_launch("dmc_known_blend");
}

extern "C" int dmc_cfg_x0(const float* x, const float* ec, const float* eu, float scale, const int64_t* t,
                          const float* ta, const float* tb, int mode, int N, int per, float p, float* eps_out,
                          float* x0_out, void* stream) {
  int npad = 1;
  while (npad < per) npad <<= 1;
  DMC_REQUIRE(npad <= 16384, "cfg_x0: %d elements per sample exceeds 16384", per);
  cfg_x0_kernel<<<N, 1024, npad * sizeof(float), dmc::as_stream(stream)>>>(x, ec, eu, scale, t, ta, tb, mode, per, npad,
                                                                          p, eps_out, x0_out);
  return dmc::check_launch("dmc_cfg_x0");
}

extern "C" int dmc_cfg_guide(int pred_type, const float* x, const float* pc, long pc_stride, const float* pu,
                             long pu_stride, float scale, float rescale, const int64_t* t, const float* sa,
                             const float* s1, int T, int N, int per, float p, float* eps_out, float* x0_out,
                             void* stream) {
  DMC_REQUIRE(pred_type == DMC_PRED_EPS || pred_type == DMC_PRED_V, "cfg_guide: unknown prediction type %d", pred_type);
  DMC_REQUIRE(T > 0 && N > 0 && per > 0, "cfg_guide: T %d, N %d, per_sample %d must be positive", T, N, per);
  DMC_REQUIRE(x && pc && pu && t && sa && s1 && x0_out, "cfg_guide: only eps_out may be NULL");
  DMC_REQUIRE(pc_stride >= per && pu_stride >= per, "cfg_guide: row strides %ld, %ld are below per_sample %d", pc_stride,
              pu_stride, per);
  DMC_REQUIRE(rescale >= 0.f && rescale <= 1.f, "cfg_guide: rescale %g is not in [0, 1]", (double)rescale);
  DMC_REQUIRE(!(p >= 1.f), "cfg_guide: p_threshold %g is not below 1", (double)p);
  int npad = 1;
  while (npad < per) npad <<= 1;
  DMC_REQUIRE(npad <= 16384, "cfg_guide: %d elements per sample exceeds 16384", per);
  const size_t lds = npad * sizeof(float) < 256 ? 256 : npad * sizeof(float);   // 16 waves x 2 double partials
  cfg_guide_kernel<<<N, 1024, lds, dmc::as_stream(stream)>>>(pred_type, x, pc, pc_stride, pu, pu_stride, scale, rescale,
                                                             t, sa, s1, T, per, npad, p, eps_out, x0_out);
  return dmc::check_launch("dmc_cfg_guide");
}

extern "C" int dmc_flow_step(const float* x, const float* pc, long pc_stride, const float* pu, long pu_stride,
                             float scale, const float* xb, const float* dprev, const int64_t* step, const float* coef,
                             int R, int N, int per, float* out, float* xb_out, float* d_out, void* stream) {
  DMC_REQUIRE(R > 0 && N > 0 && per > 0, "flow_step: R %d, N %d, per_sample %d must be positive", R, N, per);
  DMC_REQUIRE(x && pc && step && coef && out, "flow_step: x, pc, step, coef and out must not be NULL");
  DMC_REQUIRE(pc_stride >= per && (!pu || pu_stride >= per), "flow_step: row strides %ld, %ld are below per_sample %d",
              pc_stride, pu_stride, per);
  const uintptr_t bits = (uintptr_t)x | (uintptr_t)pc | (uintptr_t)pu | (uintptr_t)xb | (uintptr_t)dprev |
                         (uintptr_t)out | (uintptr_t)xb_out | (uintptr_t)d_out;   // a NULL operand adds no bits
  const bool vec = per % 4 == 0 && pc_stride % 4 == 0 && (!pu || pu_stride % 4 == 0) && (bits & 15) == 0;
  const int gx = grid_for(vec ? per / 4 : per);
  const int gy_cap = 16384 / gx > 0 ? 16384 / gx : 1;
  const dim3 grid(gx, N < gy_cap ? N : gy_cap);
  hipStream_t s = dmc::as_stream(stream);
  if (vec)
    flow_step_kernel<true><<<grid, 256, 0, s>>>(x, pc, pc_stride, pu, pu_stride, scale, xb, dprev, step, coef, R, N, per,
                                                out, xb_out, d_out);
  else
    flow_step_kernel<false><<<grid, 256, 0, s>>>(x, pc, pc_stride, pu, pu_stride, scale, xb, dprev, step, coef, R, N, per,
                                                 out, xb_out, d_out);
  return dmc::check_launch("dmc_flow_step");
}

extern "C" int dmc_flow_guide(const float* x, const float* pc, long pc_stride, const float* pu, long pu_stride,
                              float scale, float rescale, const int64_t* step, const float* coef, int R, int N, int per,
                              int threshold, float p, float* g_out, void* stream) {
  DMC_REQUIRE(R > 0 && N > 0 && per > 0, "flow_guide: R %d, N %d, per_sample %d must be positive", R, N, per);
  DMC_REQUIRE(pc && pu && step && coef && g_out, "flow_guide: pc, pu, step, coef and g_out must not be NULL");
  DMC_REQUIRE(!threshold || (x && x != g_out), "flow_guide: the threshold needs x, in a buffer other than g_out");
  DMC_REQUIRE(pc_stride >= per && pu_stride >= per, "flow_guide: row strides %ld, %ld are below per_sample %d", pc_stride,
              pu_stride, per);
  DMC_REQUIRE(rescale >= 0.f && rescale <= 1.f, "flow_guide: rescale %g is not in [0, 1]", (double)rescale);
  DMC_REQUIRE(!(p >= 1.f), "flow_guide: p_threshold %g is not below 1", (double)p);
  int npad = 1;
  while (npad < per) npad <<= 1;
  DMC_REQUIRE(npad <= 16384, "flow_guide: %d elements per sample exceeds 16384", per);
  const size_t lds = npad * sizeof(float) < 256 ? 256 : npad * sizeof(float);   // 16 waves x 2 double partials
  flow_guide_kernel<<<N, 1024, lds, dmc::as_stream(stream)>>>(x, pc, pc_stride, pu, pu_stride, scale, rescale, step, coef,
                                                              R, per, npad, threshold ? 1 : 0, p, g_out);
  return dmc::check_launch("dmc_flow_guide");
}

extern "C" int dmc_ema_update(const dmc_tensor_ref* refs, int count, float decay, void* stream) {
  if (count == 0) return 0;
  ema_kernel<<<dim3(64, count), 256, 0, dmc::as_stream(stream)>>>(refs, decay);
  return dmc::check_launch("dmc_ema_update");
}

extern "C" int dmc_clip_grad_norm(const dmc_tensor_ref* refs, int count, float max_norm, float* total_norm, float* ws,
                                  void* stream) {
  if (count == 0) return 0;
  hipStream_t s = dmc::as_stream(stream);
  float* partial = ws;
  float* coef = ws + (size_t)count * kClipSlices;
  sumsq_kernel<<<dim3(kClipSlices, count), 256, 0, s>>>(refs, partial);
  clip_coef_kernel<<<1, 256, 0, s>>>(partial, count, max_norm, total_norm, coef);
  scale_kernel<<<dim3(64, count), 256, 0, s>>>(refs, coef);
  return dmc::check_launch("dmc_clip_grad_norm");
}

extern "C" int dmc_unpack_output(int dtype, const void* src, int ld, int N, int C, int H, int W, float* dst,
                                 void* stream) {
  const long total = (long)N * C * H * W;
  hipStream_t s = dmc::as_stream(stream);
  if (dtype == DMC_F32) unpack_kernel<float><<<grid_for(total), 256, 0, s>>>((const float*)src, ld, N, C, H, W, dst);
  else unpack_kernel<bf16_t><<<grid_for(total), 256, 0, s>>>((const bf16_t*)src, ld, N, C, H, W, dst);
  return dmc::check_launch("dmc_unpack_output");
}

extern "C" int dmc_add(int dtype, void* y, const void* x, long n, void* stream) {
  hipStream_t s = dmc::as_stream(stream);
  if (dtype == DMC_F32) add_kernel<float><<<grid_for(n), 256, 0, s>>>((float*)y, (const float*)x, n);
  else add_kernel<bf16_t><<<grid_for(n), 256, 0, s>>>((bf16_t*)y, (const bf16_t*)x, n);
  return dmc::check_launch("dmc_add");
}

extern "C" int dmc_upsample2x_nhwc(int dtype, const void* x, int N, int H, int W, int C, int ld, void* y, int ldy,
                                   void* stream) {
  const int esz = dtype == DMC_F32 ? 4 : 2;
  DMC_REQUIRE((C * esz) % 16 == 0 && (ld * esz) % 16 == 0 && (ldy * esz) % 16 == 0 && ld >= C && ldy >= C,
              "upsample2x: channels/pitches must be 16-byte multiples (C=%d ld=%d ldy=%d)", C, ld, ldy);
  const long total = (long)N * H * W * (C * esz / 16);
  if (total == 0) return 0;
  upsample2x_nhwc_kernel<<<grid_for(total, 256, 16384), 256, 0, dmc::as_stream(stream)>>>(
      (const char*)x, N, H, W, C * esz, ld * esz, (char*)y, ldy * esz);
  return dmc::check_launch("dmc_upsample2x_nhwc");
}

extern "C" int dmc_silu_fwd(const float* x, float* y, long n, void* stream) {
  silu_kernel<<<grid_for(n), 256, 0, dmc::as_stream(stream)>>>(x, y, n);
  return dmc::check_launch("dmc_silu_fwd");
}

extern "C" int dmc_grad_norm_flat(const float* g, long n, float max_norm, float* total_norm, float* coef, float* ws,
                                  void* stream) {
  DMC_REQUIRE(((uintptr_t)g & 15) == 0, "grad_norm_flat: buffer must be 16-byte aligned");
  hipStream_t s = dmc::as_stream(stream);
  flat_sumsq_kernel<<<kNormBlocks, 256, 0, s>>>(g, n, ws);
  flat_norm_final<<<1, 256, 0, s>>>(ws, max_norm, total_norm, coef);
  return dmc::check_launch("dmc_grad_norm_flat");
}

extern "C" int dmc_adamw_flat(float* p, const float* g, float* m, float* v, float* ema, long n, const float* coef,
                              float wd_mul, float lerp_w, float beta2, float one_minus_beta2, float eps,
                              float neg_step_size, float bc2_sqrt, float ema_decay, float ema_one_minus, void* stream) {
  DMC_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0,
              "adamw_flat: buffers must be 16-byte aligned");
  AdamWArgs a{p, g, m, v, ema, coef, n, wd_mul, lerp_w, beta2, one_minus_beta2, neg_step_size, bc2_sqrt, eps,
              ema_decay, ema_one_minus, nullptr};
  adamw_flat_kernel<<<grid_for(n / 4 + 1, 256, 4096), 256, 0, dmc::as_stream(stream)>>>(a);
  return dmc::check_launch("dmc_adamw_flat");
}

extern "C" int dmc_adamw_flat_dev(float* p, const float* g, float* m, float* v, float* ema, long n, const float* coef,
                                  const float* hyper, void* stream) {
  DMC_REQUIRE((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) & 15) == 0,
              "adamw_flat_dev: buffers must be 16-byte aligned");
  DMC_REQUIRE(hyper != nullptr, "adamw_flat_dev: hyper must point to 9 device floats");
  AdamWArgs a{p, g, m, v, ema, coef, n, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, hyper};
  adamw_flat_kernel<<<grid_for(n / 4 + 1, 256, 4096), 256, 0, dmc::as_stream(stream)>>>(a);
  return dmc::check_launch("dmc_adamw_flat_dev");
}
