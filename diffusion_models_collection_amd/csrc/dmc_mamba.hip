// The Mamba token mixer of the DiM backbone (models/dim.py of sunyzhi55/Diffusion_Models_Collection, MambaBlock with
// mamba_ssm.Mamba(d_state=16, d_conv=4, expand=2)) for gfx950: what the implicit-GEMM kernels do not cover.
//
//   causal_conv_silu_fwd/bwd   u_t = SiLU(bias + sum_k w[c][k] * x_{t-3+k}) over the tokens of one image (x_{<0} = 0:
//                              the token axis restarts at every image of the flat [T = B*L, E] rows)
//   selective_scan_fwd         delta = softplus(dpre + dt_bias); s_t = exp(delta_t A) s_{t-1} + delta_t Bm_t u_t;
//                              y_t = (sum_n Cm_t[n] s_t[n] + D u_t) * SiLU(z_t)            (A = -exp(A_log))
//   selective_scan_bwd         the reverse recurrence, with the states recomputed chunk by chunk
//
// Scan layout: one lane per (channel, state), N = 16 states = one 16-lane row, so sum_n is a row reduction and a wave
// holds 4 channels; a block of 256 threads owns 16 channels of one chunk of kScanChunk tokens of one image. The
// recurrence is linear in the state, so the token axis is cut into chunks:
//   pass 1  every chunk runs from a zero state and emits (P = product of its decays, S = its final state)
//   pass 2  one thread per (image, channel, state) carries s_in[k+1] = P[k] s_in[k] + S[k] over the chunks, in order
//   pass 3  every chunk reruns from its true entry state s_in[k] and writes y
// s_in (the states at the chunk boundaries, fp32) is all the backward keeps of the states; the backward has the same
// three passes in reverse for the state gradient and recomputes the states of a chunk into LDS.
// Every reduction has a fixed order (row / wave shuffles, then LDS or a partial slab summed by a second kernel):
// no float atomics, bitwise reproducible from run to run. The state and all accumulation are fp32, and so are the
// delta pre-activation and Bm / Cm rows the scan reads (their GEMMs store fp32 also in bf16 mode); u, z, y and the
// gradient rows are in the storage dtype.
#include "dmc_common.h"
#include "dmc_internal.h"

namespace {

constexpr int kScanChunk = 32;   // tokens per chunk
constexpr int kN = 16;           // states per channel (d_state)
constexpr int kCB = 16;          // channels per 256-thread block pass
constexpr int kBwdSub = 4;       // channel groups of kCB a backward block walks (its dBm / dCm partial covers 64 channels)

inline int grid_for(long n, int block = 256, int cap = 8192) {
  long b = (n + block - 1) / block;
  if (b < 1) b = 1;
  return (int)(b < cap ? b : cap);
}

DMC_DEV float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }     // torch softplus, threshold 20
DMC_DEV float softplus_grad(float x) { return x > 20.f ? 1.f : 1.f / (1.f + expf(-x)); }
DMC_DEV float sigmoid_acc(float z) { return 1.f / (1.f + expf(-z)); }
DMC_DEV float row16_sum(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------------------------
// causal depthwise conv (k = 4) + SiLU
template <typename T>
DMC_DEV float conv_pre(const void* x, int ld_x, const float* w4, float bias, size_t img_row0, int l, int c) {
  float acc = bias;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ls = l - 3 + k;
    if (ls >= 0) acc += w4[k] * ld_as_f<T>(x, (img_row0 + ls) * (size_t)ld_x + c);
  }
  return acc;
}

// Scan orders (ORD = true): logical token l of an image is the physical row order_token(l) of it. The masks
// (x_{t<0} = 0, l + j < L) are tests on logical positions and come before any mapping; a lane divides once per
// element (forward) or per segment (backward) -- a multiplication by the host's reciprocal, dmc::order_line -- and then
// carries (line a, place b) by +-1.
using dmc::ScanOrd;
DMC_DEV void ord_step(int inner, int dq, int& a, int& b) {
  b += dq;
  if (b < 0) { b = inner - 1; --a; }
  else if (b >= inner) { b = 0; ++a; }
}

// r[k] = the physical row (within the image) of logical token l - 3 + k; entries before the image's start stay 0
// and are never read
DMC_DEV void ord_rows4(ScanOrd o, int L, int l, int r[4]) {
  const int inner = dmc::order_inner(o), dq = (o.order & 1) ? 1 : -1;    // one logical step back, in q
  const int q = (o.order & 1) ? L - 1 - l : l;
  int a, b;
  dmc::order_line(o, q, a, b);
  r[3] = dmc::order_token_ab(o, a, b);
#pragma unroll
  for (int k = 2; k >= 0; --k) {
    r[k] = 0;
    if (l - 3 + k >= 0) {
      ord_step(inner, dq, a, b);
      r[k] = dmc::order_token_ab(o, a, b);
    }
  }
}

// conv_pre with the rows of the logical tokens l - 3 .. l given (r[k], within the image)
template <typename T>
DMC_DEV float conv_pre_rows(const void* x, int ld_x, const float* w4, float bias, size_t img_row0, const int* r, int l,
                            int c) {
  float acc = bias;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int ls = l - 3 + k;
    if (ls >= 0) acc += w4[k] * ld_as_f<T>(x, (img_row0 + r[k]) * (size_t)ld_x + c);
  }
  return acc;
}

template <typename T, bool ORD>
__global__ void causal_conv_fwd_kernel(const void* x, int ld_x, const float* w, const float* bias, int B, int L, int E,
                                       void* u, int ld_u, ScanOrd o) {
  const long total = (long)B * L * E;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % E);
    const long row = i / E;
    const int l = (int)(row % L);
    const float w4[4] = {w[c * 4], w[c * 4 + 1], w[c * 4 + 2], w[c * 4 + 3]};
    float p;
    size_t orow = (size_t)row;
    if (ORD) {
      int r[4];
      ord_rows4(o, L, l, r);
      p = conv_pre_rows<T>(x, ld_x, w4, bias[c], (size_t)(row - l), r, l, c);
      orow = (size_t)(row - l) + r[3];
    } else {
      p = conv_pre<T>(x, ld_x, w4, bias[c], (size_t)(row - l), l, c);
    }
    st_from_f<T>(u, orow * ld_u + c, p * sigmoid_acc(p));
  }
}

// One wave per (64 channels, token segment, image): a lane walks its channel over the segment's tokens. For token l
// it recomputes dpre_{l..l+3} = du * SiLU'(pre) (7 x rows, 4 du rows, L2-resident), writes
// dx_l = sum_j w[3-j] dpre_{l+j} and accumulates dw[k] += dpre_l x_{l-3+k}, dbias += dpre_l in token order; the
// segment sums go to ws[b][seg][5][E] and colsum5_kernel adds them in (image, segment) order.
// ORD: the segment bounds, the loop and ws stay logical; win[m] is the physical row of logical token l - 3 + m (the 7
// the step reads), shifted by one per token, the new last entry stepped from the cursor (ca, cb) without a division.
template <typename T, bool ORD>
__global__ __launch_bounds__(64) void causal_conv_bwd_kernel(const void* du, int ld_du, const void* x, int ld_x,
                                                             const float* w, const float* bias, int L, int E,
                                                             void* dx, int ld_dx, float* ws, ScanOrd o) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= E) return;
  const int S = gridDim.y, sp = blockIdx.y, b = blockIdx.z;
  const int l0 = (int)((long)L * sp / S), l1 = (int)((long)L * (sp + 1) / S);
  const size_t r0 = (size_t)b * L;
  const float w4[4] = {w[c * 4], w[c * 4 + 1], w[c * 4 + 2], w[c * 4 + 3]};
  const float bs = bias[c];
  float aw[4] = {0.f, 0.f, 0.f, 0.f}, ab = 0.f;
  int win[7] = {0, 0, 0, 0, 0, 0, 0}, ca = 0, cb = 0;
  const int inner = ORD ? dmc::order_inner(o) : 1, dq = (o.order & 1) ? -1 : 1;   // one logical step forward, in q
  if (ORD && l0 < l1) {
    const int ps = l0 > 3 ? l0 - 3 : 0;      // the first logical token the segment reads
    const int q = (o.order & 1) ? L - 1 - ps : ps;
    dmc::order_line(o, q, ca, cb);
#pragma unroll
    for (int m = 0; m < 6; ++m) {
      const int p = l0 - 3 + m;
      if (p >= ps && p < L) {
        win[m] = dmc::order_token_ab(o, ca, cb);
        ord_step(inner, dq, ca, cb);
      }
    }
  }
  for (int l = l0; l < l1; ++l) {
    if (ORD) {
      win[6] = 0;
      if (l + 3 < L) {
        win[6] = dmc::order_token_ab(o, ca, cb);
        ord_step(inner, dq, ca, cb);
      }
    }
    float dp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dp[j] = 0.f;
      if (l + j < L) {
        const float p = ORD ? conv_pre_rows<T>(x, ld_x, w4, bs, r0, win + j, l + j, c)
                            : conv_pre<T>(x, ld_x, w4, bs, r0, l + j, c);
        const float sg = sigmoid_acc(p);
        const size_t rd = ORD ? r0 + win[j + 3] : r0 + l + j;
        dp[j] = ld_as_f<T>(du, rd * (size_t)ld_du + c) * (sg * (1.f + p * (1.f - sg)));
      }
    }
    const size_t rx = ORD ? r0 + win[3] : r0 + l;
    st_from_f<T>(dx, rx * (size_t)ld_dx + c, ((w4[3] * dp[0] + w4[2] * dp[1]) + w4[1] * dp[2]) + w4[0] * dp[3]);
    ab += dp[0];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int ls = l - 3 + k;
      if (ls >= 0) aw[k] += dp[0] * ld_as_f<T>(x, (ORD ? r0 + win[k] : r0 + ls) * (size_t)ld_x + c);
    }
    if (ORD) {
#pragma unroll
      for (int m = 0; m < 6; ++m) win[m] = win[m + 1];
    }
  }
  float* seg = ws + (size_t)(b * S + sp) * 5 * E;
#pragma unroll
  for (int k = 0; k < 4; ++k) seg[(size_t)k * E + c] = aw[k];
  seg[(size_t)4 * E + c] = ab;
}

// dw[c][k] = sum over q (in order) of ws[q][k][c], dbias[c] = sum of ws[q][4][c]
__global__ void colsum5_kernel(const float* ws, int Q, int E, float* dw, float* dbias) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 5 * E; i += gridDim.x * blockDim.x) {
    const int k = i / E, c = i - k * E;
    float s = 0.f;
    for (int q = 0; q < Q; ++q) s += ws[((size_t)q * 5 + k) * E + c];
    if (k < 4) dw[c * 4 + k] = s;
    else dbias[c] = s;
  }
}

int conv_splits(int B, int L, int E) {
  const int cg = (E + 63) / 64;
  int S = (2048 + B * cg - 1) / (B * cg);
  if (S > L / 8) S = L / 8;
  return S < 1 ? 1 : (S > 256 ? 256 : S);
}

// ---------------------------------------------------------------------------------------------------------------
// selective scan
struct ScanArgs {
  const void *u, *z;              // storage dtype T
  const float *dpre, *Bm, *Cm;    // fp32 whatever T is: a bf16 delta / Bm / Cm costs the recurrence its accuracy
  int ld_u, ld_z, ld_dp, ld_bc;
  const float *A_log, *D, *dt_bias;
  int L, E, K;
};

// The token rows a thread of a scan block stages and stores: element i = tid, tid + 256 of a [kScanChunk][16] tile is
// token tt = i >> 4 of the chunk, so a thread touches the two tokens tid >> 4 and 16 + (tid >> 4). ORD = false: row
// base + tt. ORD = true: the physical rows of those two logical tokens, mapped once per block (two order_token
// per thread, nothing in the token loops); the chunk index, t0 and every per-chunk slab index stay logical.
template <bool ORD>
struct ChunkRows {
  size_t base, r0, r1;
  DMC_DEV ChunkRows(ScanOrd o, size_t img_row0, int t0, int len, int tid) : base(img_row0 + t0), r0(0), r1(0) {
    if (ORD) {
      const int tl = tid >> 4;
      r0 = img_row0 + (tl < len ? dmc::order_token(o, t0 + tl) : 0);
      r1 = img_row0 + (tl + 16 < len ? dmc::order_token(o, t0 + tl + 16) : 0);
    }
  }
  DMC_DEV size_t operator()(int i, int tt) const { return ORD ? (i < 256 ? r0 : r1) : base + tt; }
};

// MODE 0: the chunk from a zero state -> (P, S).  MODE 1: the chunk from s_in -> y (gated).
template <typename T, int MODE, bool ORD>
__global__ __launch_bounds__(256) void scan_fwd_kernel(ScanArgs a, const float* s_in, float* Pout, float* Sout, void* y,
                                                       int ld_y, ScanOrd o) {
  __shared__ float sdelta[kScanChunk][kCB], su[kScanChunk][kCB], sz[kScanChunk][kCB], sy[kScanChunk][kCB];
  __shared__ float sB[kScanChunk][kN], sC[kScanChunk][kN];
  const int tid = threadIdx.x, cl = tid >> 4, n = tid & 15;
  const int c0 = blockIdx.x * kCB, k = blockIdx.y, b = blockIdx.z;
  const int t0 = k * kScanChunk, len = min(kScanChunk, a.L - t0);
  const ChunkRows<ORD> R(o, (size_t)b * a.L, t0, len, tid);
  for (int i = tid; i < kScanChunk * kCB; i += 256) {
    const int tt = i >> 4, cc = i & 15, ce = c0 + cc;
    float d = 0.f, uu = 0.f, zz = 0.f, bb = 0.f, cv = 0.f;
    if (tt < len) {
      if (ce < a.E) {
        d = softplus_f(ld_as_f<float>(a.dpre, R(i, tt) * a.ld_dp + ce) + a.dt_bias[ce]);
        uu = ld_as_f<T>(a.u, R(i, tt) * a.ld_u + ce);
        if (MODE == 1) zz = ld_as_f<T>(a.z, R(i, tt) * a.ld_z + ce);
      }
      bb = ld_as_f<float>(a.Bm, R(i, tt) * a.ld_bc + cc);
      if (MODE == 1) cv = ld_as_f<float>(a.Cm, R(i, tt) * a.ld_bc + cc);
    }
    sdelta[tt][cc] = d; su[tt][cc] = uu; sz[tt][cc] = zz; sB[tt][cc] = bb; sC[tt][cc] = cv;
  }
  __syncthreads();
  const int c = c0 + cl;
  const bool valid = c < a.E;
  const size_t si = (((size_t)b * a.K + k) * a.E + (valid ? c : 0)) * kN + n;
  const float A = valid ? -expf(a.A_log[c * kN + n]) : 0.f;
  const float Dc = valid ? a.D[c] : 0.f;
  float s = (MODE == 1 && s_in && valid) ? s_in[si] : 0.f;
  float P = 1.f;
  for (int tt = 0; tt < len; ++tt) {
    const float d = sdelta[tt][cl], uu = su[tt][cl];
    const float da = expf(d * A);
    s = da * s + (d * sB[tt][n]) * uu;
    if (MODE == 0) {
      P *= da;
    } else {
      const float yv = row16_sum(s * sC[tt][n]);
      if (n == 0) {
        const float zz = sz[tt][cl];
        sy[tt][cl] = (yv + Dc * uu) * (zz * sigmoid_acc(zz));
      }
    }
  }
  if (MODE == 0) {
    if (valid) { Pout[si] = P; Sout[si] = s; }
    return;
  }
  __syncthreads();
  for (int i = tid; i < len * kCB; i += 256) {
    const int tt = i >> 4, cc = i & 15;
    if (c0 + cc < a.E) st_from_f<T>(y, R(i, tt) * ld_y + c0 + cc, sy[tt][cc]);
  }
}

// carry[k] for every (image, channel, state): forward  in[0] = 0, in[k+1] = P[k] in[k] + S[k];
// reverse in[K-1] = 0, in[k-1] = P[k] in[k] + S[k]
__global__ void scan_carry_kernel(const float* P, const float* S, float* in, int B, int K, long EN, int reverse) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (long)B * EN; i += (long)gridDim.x * blockDim.x) {
    const long b = i / EN, j = i - b * EN;
    float carry = 0.f;
    for (int q = 0; q < K; ++q) {
      const int k = reverse ? K - 1 - q : q;
      const size_t o = ((size_t)b * K + k) * EN + j;
      in[o] = carry;
      carry = P[o] * carry + S[o];
    }
  }
}

// Backward pass 1: the state-gradient recurrence of one chunk from a zero carry:
// g_t = Cm_t dyv_t + carry, carry = a_t g_t  ->  (P = product of the decays, S = the carry leaving the chunk's start)
template <typename T, bool ORD>
__global__ __launch_bounds__(256) void scan_bwd_local_kernel(ScanArgs a, const void* dy, int ld_dy, float* Pout,
                                                             float* Sout, ScanOrd o) {
  __shared__ float sdelta[kScanChunk][kCB], sdyv[kScanChunk][kCB], sC[kScanChunk][kN];
  const int tid = threadIdx.x, cl = tid >> 4, n = tid & 15;
  const int c0 = blockIdx.x * kCB, k = blockIdx.y, b = blockIdx.z;
  const int t0 = k * kScanChunk, len = min(kScanChunk, a.L - t0);
  const ChunkRows<ORD> R(o, (size_t)b * a.L, t0, len, tid);
  for (int i = tid; i < kScanChunk * kCB; i += 256) {
    const int tt = i >> 4, cc = i & 15, ce = c0 + cc;
    float d = 0.f, g = 0.f, cv = 0.f;
    if (tt < len) {
      if (ce < a.E) {
        d = softplus_f(ld_as_f<float>(a.dpre, R(i, tt) * a.ld_dp + ce) + a.dt_bias[ce]);
        const float zz = ld_as_f<T>(a.z, R(i, tt) * a.ld_z + ce);
        g = ld_as_f<T>(dy, R(i, tt) * ld_dy + ce) * (zz * sigmoid_acc(zz));
      }
      cv = ld_as_f<float>(a.Cm, R(i, tt) * a.ld_bc + cc);
    }
    sdelta[tt][cc] = d; sdyv[tt][cc] = g; sC[tt][cc] = cv;
  }
  __syncthreads();
  const int c = c0 + cl;
  if (c >= a.E) return;
  const float A = -expf(a.A_log[c * kN + n]);
  float carry = 0.f, P = 1.f;
  for (int tt = len - 1; tt >= 0; --tt) {
    const float da = expf(sdelta[tt][cl] * A);
    carry = da * (sC[tt][n] * sdyv[tt][cl] + carry);
    P *= da;
  }
  const size_t si = (((size_t)b * a.K + k) * a.E + c) * kN + n;
  Pout[si] = P; Sout[si] = carry;
}

// Backward pass 3: a block walks up to kBwdSub groups of 16 channels over one chunk. Per group: stage the chunk's
// operands, recompute the states from s_in into LDS (stash[t] = s_{t-1}), then the reverse recurrence from g_in.
// Outputs: du, dz, ddpre rows (through LDS, coalesced); per-(image, chunk) partials of dA_log [E][N] and dD [E];
// per-token partials of dBm / dCm over the block's channels: part[row][gridDim.x][2][N] (row physical:
// scan_bc_reduce_kernel reads per physical row).
template <typename T, bool ORD>
__global__ __launch_bounds__(256) void scan_bwd_kernel(ScanArgs a, const void* dy, int ld_dy, const float* s_in,
                                                       const float* g_in, void* du, int ld_du, void* dz, int ld_dz,
                                                       void* ddp, int ld_ddp, float* slabA, float* slabD,
                                                       float* part, ScanOrd o) {
  __shared__ float stash[kScanChunk][256];
  __shared__ float redB[4][kScanChunk][kN], redC[4][kScanChunk][kN];
  __shared__ float sdelta[kScanChunk][kCB], su[kScanChunk][kCB], sdyv[kScanChunk][kCB], sdzf[kScanChunk][kCB],
      sdsp[kScanChunk][kCB];
  __shared__ float sB[kScanChunk][kN], sC[kScanChunk][kN];
  const int tid = threadIdx.x, cl = tid >> 4, n = tid & 15, wave = tid >> 6, lane = tid & 63;
  const int k = blockIdx.y, b = blockIdx.z;
  const int t0 = k * kScanChunk, len = min(kScanChunk, a.L - t0);
  const ChunkRows<ORD> R(o, (size_t)b * a.L, t0, len, tid);
  for (int i = tid; i < kScanChunk * kN; i += 256) {
    const int tt = i >> 4, cc = i & 15;
    float bb = 0.f, cv = 0.f;
    if (tt < len) {
      bb = ld_as_f<float>(a.Bm, R(i, tt) * a.ld_bc + cc);
      cv = ld_as_f<float>(a.Cm, R(i, tt) * a.ld_bc + cc);
    }
    sB[tt][cc] = bb; sC[tt][cc] = cv;
  }
  for (int i = tid; i < 4 * kScanChunk * kN; i += 256) { (&redB[0][0][0])[i] = 0.f; (&redC[0][0][0])[i] = 0.f; }
  for (int sub = 0; sub < kBwdSub; ++sub) {
    const int c0 = (blockIdx.x * kBwdSub + sub) * kCB;
    if (c0 >= a.E) break;          // uniform over the block
    __syncthreads();               // the previous group's LDS rows are stored; B / C / red are initialised
    for (int i = tid; i < kScanChunk * kCB; i += 256) {
      const int tt = i >> 4, cc = i & 15, ce = c0 + cc;
      float d = 0.f, uu = 0.f, gv = 0.f, gz = 0.f, sp = 0.f;
      if (tt < len && ce < a.E) {
        const float pre = ld_as_f<float>(a.dpre, R(i, tt) * a.ld_dp + ce) + a.dt_bias[ce];
        d = softplus_f(pre);
        sp = softplus_grad(pre);
        uu = ld_as_f<T>(a.u, R(i, tt) * a.ld_u + ce);
        const float zz = ld_as_f<T>(a.z, R(i, tt) * a.ld_z + ce);
        const float g = ld_as_f<T>(dy, R(i, tt) * ld_dy + ce);
        const float sg = sigmoid_acc(zz);
        gv = g * (zz * sg);
        gz = g * (sg * (1.f + zz * (1.f - sg)));
      }
      sdelta[tt][cc] = d; su[tt][cc] = uu; sdyv[tt][cc] = gv; sdzf[tt][cc] = gz; sdsp[tt][cc] = sp;
    }
    __syncthreads();
    const int c = c0 + cl;
    const bool valid = c < a.E;
    const size_t si = (((size_t)b * a.K + k) * a.E + (valid ? c : 0)) * kN + n;
    const float A = valid ? -expf(a.A_log[c * kN + n]) : 0.f;
    const float Dc = valid ? a.D[c] : 0.f;
    float s = (s_in && valid) ? s_in[si] : 0.f;
    for (int tt = 0; tt < len; ++tt) {
      stash[tt][tid] = s;
      const float d = sdelta[tt][cl];
      s = expf(d * A) * s + (d * sB[tt][n]) * su[tt][cl];
    }
    float carry = (g_in && valid) ? g_in[si] : 0.f;
    float accA = 0.f, accD = 0.f;
    for (int tt = len - 1; tt >= 0; --tt) {
      const float d = sdelta[tt][cl], uu = su[tt][cl], gy = sdyv[tt][cl];
      const float bn = sB[tt][n], cn = sC[tt][n];
      const float da = expf(d * A);
      const float sp = stash[tt][tid];
      const float st = da * sp + (d * bn) * uu;
      const float g = cn * gy + carry;
      const float gda = g * sp * da;        // d loss / d (delta * A)
      accA += gda * d;
      carry = da * g;
      const float yv = row16_sum(st * cn);
      const float vdelta = row16_sum(gda * A + g * bn * uu);
      const float vu = row16_sum(g * d * bn);
      float vB = g * d * uu, vC = gy * st;
      vB += __shfl_xor(vB, 16, 64); vB += __shfl_xor(vB, 32, 64);
      vC += __shfl_xor(vC, 16, 64); vC += __shfl_xor(vC, 32, 64);
      if (lane < 16) { redB[wave][tt][n] += vB; redC[wave][tt][n] += vC; }
      if (n == 0) {
        accD += gy * uu;
        sdzf[tt][cl] = (yv + Dc * uu) * sdzf[tt][cl];   // dz
        su[tt][cl] = vu + gy * Dc;                      // du
        sdelta[tt][cl] = vdelta * sdsp[tt][cl];         // d (delta pre-activation)
      }
    }
    if (valid) {
      slabA[si] = accA * A;                             // dA_log = dA * A
      if (n == 0) slabD[((size_t)b * a.K + k) * a.E + c] = accD;
    }
    __syncthreads();
    for (int i = tid; i < len * kCB; i += 256) {
      const int tt = i >> 4, cc = i & 15, ce = c0 + cc;
      if (ce < a.E) {
        st_from_f<T>(du, R(i, tt) * ld_du + ce, su[tt][cc]);
        st_from_f<T>(dz, R(i, tt) * ld_dz + ce, sdzf[tt][cc]);
        st_from_f<T>(ddp, R(i, tt) * ld_ddp + ce, sdelta[tt][cc]);
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < len * kN; i += 256) {
    const int tt = i >> 4, nn = i & 15;
    float* pt = part + (R(i, tt) * gridDim.x + blockIdx.x) * 2 * kN;
    pt[nn] = ((redB[0][tt][nn] + redB[1][tt][nn]) + redB[2][tt][nn]) + redB[3][tt][nn];
    pt[kN + nn] = ((redC[0][tt][nn] + redC[1][tt][nn]) + redC[2][tt][nn]) + redC[3][tt][nn];
  }
}

// dbc[row][col0 + j] = sum over the G channel blocks (in order) of part[row][g][j], j < 2N; the pitch padding behind
// them is zeroed (the x_proj gradient GEMMs read whole chunks)
template <typename T>
__global__ void scan_bc_reduce_kernel(const float* part, long rows, int G, void* dbc, int ld, int col0) {
  const int w = ld - col0;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < rows * w; i += (long)gridDim.x * blockDim.x) {
    const long r = i / w;
    const int j = (int)(i - r * w);
    float s = 0.f;
    if (j < 2 * kN)
      for (int g = 0; g < G; ++g) s += part[((size_t)r * G + g) * 2 * kN + j];
    st_from_f<T>(dbc, (size_t)r * ld + col0 + j, s);
  }
}

// out[i] = sum over q (in order) of slab[q][i]
__global__ void slab_sum_kernel(const float* slab, int Q, long n, float* out) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int q = 0; q < Q; ++q) s += slab[(size_t)q * n + i];
    out[i] = s;
  }
}

int scan_check(const char* what, int dtype, int B, int L, int E, int N) {
  DMC_REQUIRE(dtype == DMC_F32 || dtype == DMC_BF16, "%s: dtype %d", what, dtype);
  DMC_REQUIRE(N == kN, "%s: d_state %d (the scan kernels hold one state per lane of a 16-lane row: 16 only)", what, N);
  DMC_REQUIRE(B > 0 && L > 0 && E > 0 && (long)B * L * E < (1L << 31), "%s: B %d L %d E %d", what, B, L, E);
  DMC_REQUIRE(B <= 65535 && (L + kScanChunk - 1) / kScanChunk <= 65535, "%s: grid B %d L %d", what, B, L);
  return 0;
}

// (h, w, order) of an _ord entry point -> L = h * w and the launch constant
int order_check(const char* what, int h, int w, int order, int* L, ScanOrd* o) {
  DMC_REQUIRE(h > 0 && w > 0 && (long)h * w < (1L << 31), "%s: token grid %d x %d", what, h, w);
  DMC_REQUIRE(order >= 0 && order < 8, "%s: scan order %d (a 3-bit code: 1 reverse, 2 column-major, 4 snake)", what,
              order);
  *L = h * w;
  *o = dmc::make_scan_ord(h, w, order);
  return 0;
}

template <bool ORD>
int conv_fwd_launch(const char* what, int dtype, const void* x, int ld_x, const float* w, const float* bias, int B, int L,
                    int E, void* u, int ld_u, ScanOrd o, void* stream) {
  DMC_REQUIRE(B > 0 && L > 0 && E > 0 && ld_x >= E && ld_u >= E, "causal_conv_fwd: B %d L %d E %d", B, L, E);
  hipStream_t s = dmc::as_stream(stream);
  const int g = grid_for((long)B * L * E);
  if (dtype == DMC_F32) causal_conv_fwd_kernel<float, ORD><<<g, 256, 0, s>>>(x, ld_x, w, bias, B, L, E, u, ld_u, o);
  else causal_conv_fwd_kernel<bf16_t, ORD><<<g, 256, 0, s>>>(x, ld_x, w, bias, B, L, E, u, ld_u, o);
  return dmc::check_launch(what);
}

template <bool ORD>
int conv_bwd_launch(const char* what, int dtype, const void* du, int ld_du, const void* x, int ld_x, const float* w,
                    const float* bias, int B, int L, int E, void* dx, int ld_dx, float* dw, float* dbias,
                    void* workspace, ScanOrd o, void* stream) {
  DMC_REQUIRE(B > 0 && B <= 65535 && L > 0 && E > 0 && ld_x >= E && ld_du >= E && ld_dx >= E && workspace,
              "causal_conv_bwd: B %d L %d E %d", B, L, E);
  hipStream_t s = dmc::as_stream(stream);
  const int S = conv_splits(B, L, E);
  const dim3 g((E + 63) / 64, S, B);
  float* ws = (float*)workspace;
  if (dtype == DMC_F32)
    causal_conv_bwd_kernel<float, ORD><<<g, 64, 0, s>>>(du, ld_du, x, ld_x, w, bias, L, E, dx, ld_dx, ws, o);
  else
    causal_conv_bwd_kernel<bf16_t, ORD><<<g, 64, 0, s>>>(du, ld_du, x, ld_x, w, bias, L, E, dx, ld_dx, ws, o);
  colsum5_kernel<<<grid_for(5L * E), 256, 0, s>>>(ws, B * S, E, dw, dbias);
  return dmc::check_launch(what);
}

template <bool ORD>
int scan_fwd_launch(const char* what, int dtype, const void* u, int ld_u, const void* z, int ld_z, const float* dpre,
                    int ld_dp, const float* Bm, const float* Cm, int ld_bc, const float* A_log, const float* D,
                    const float* dt_bias, int B, int L, int E, int N, float* states, void* workspace, void* y, int ld_y,
                    ScanOrd o, void* stream) {
  if (scan_check("selective_scan_fwd", dtype, B, L, E, N)) return 1;
  const int K = (L + kScanChunk - 1) / kScanChunk;
  DMC_REQUIRE(K == 1 || (states && workspace), "selective_scan_fwd: %d chunks need the state and workspace buffers", K);
  hipStream_t s = dmc::as_stream(stream);
  const ScanArgs a{u, z, dpre, Bm, Cm, ld_u, ld_z, ld_dp, ld_bc, A_log, D, dt_bias, L, E, K};
  const dim3 g((E + kCB - 1) / kCB, K, B);
  const size_t st = (size_t)B * K * E * N;
  float* P = (float*)workspace;
  float* S = P ? P + st : nullptr;
  const float* s0 = K > 1 ? states : nullptr;
  if (K > 1) {
    if (dtype == DMC_F32) scan_fwd_kernel<float, 0, ORD><<<g, 256, 0, s>>>(a, nullptr, P, S, nullptr, 0, o);
    else scan_fwd_kernel<bf16_t, 0, ORD><<<g, 256, 0, s>>>(a, nullptr, P, S, nullptr, 0, o);
    scan_carry_kernel<<<grid_for((long)B * E * N), 256, 0, s>>>(P, S, states, B, K, (long)E * N, 0);
  }
  if (dtype == DMC_F32) scan_fwd_kernel<float, 1, ORD><<<g, 256, 0, s>>>(a, s0, nullptr, nullptr, y, ld_y, o);
  else scan_fwd_kernel<bf16_t, 1, ORD><<<g, 256, 0, s>>>(a, s0, nullptr, nullptr, y, ld_y, o);
  return dmc::check_launch(what);
}

template <bool ORD>
int scan_bwd_launch(const char* what, int dtype, const void* dy, int ld_dy, const void* u, int ld_u, const void* z,
                    int ld_z, const float* dpre, int ld_dp, const float* Bm, const float* Cm, int ld_bc,
                    const float* A_log, const float* D, const float* dt_bias, int B, int L, int E, int N,
                    const float* states, void* workspace, void* du, int ld_du, void* dz, int ld_dz, void* ddpre,
                    int ld_ddp, void* dbc, int ld_dbc, int bc_col, float* dA_log, float* dD, ScanOrd o, void* stream) {
  if (scan_check("selective_scan_bwd", dtype, B, L, E, N)) return 1;
  const int K = (L + kScanChunk - 1) / kScanChunk;
  DMC_REQUIRE(workspace && (K == 1 || states), "selective_scan_bwd: workspace / chunk states");
  DMC_REQUIRE(bc_col >= 0 && ld_dbc >= bc_col + 2 * N, "selective_scan_bwd: dbc pitch %d column %d", ld_dbc, bc_col);
  hipStream_t s = dmc::as_stream(stream);
  const ScanArgs a{u, z, dpre, Bm, Cm, ld_u, ld_z, ld_dp, ld_bc, A_log, D, dt_bias, L, E, K};
  const size_t st = (size_t)B * K * E * N;
  const int G = (E + kCB * kBwdSub - 1) / (kCB * kBwdSub);
  float* P = (float*)workspace;
  float* S = P + st;
  float* gin = S + st;
  float* slabA = gin + st;
  float* slabD = slabA + st;
  float* part = slabD + (size_t)B * K * E;
  const float* s0 = K > 1 ? states : nullptr;
  if (K > 1) {
    const dim3 g1((E + kCB - 1) / kCB, K, B);
    if (dtype == DMC_F32) scan_bwd_local_kernel<float, ORD><<<g1, 256, 0, s>>>(a, dy, ld_dy, P, S, o);
    else scan_bwd_local_kernel<bf16_t, ORD><<<g1, 256, 0, s>>>(a, dy, ld_dy, P, S, o);
    scan_carry_kernel<<<grid_for((long)B * E * N), 256, 0, s>>>(P, S, gin, B, K, (long)E * N, 1);
  }
  const dim3 g(G, K, B);
  const float* gi = K > 1 ? gin : nullptr;
  if (dtype == DMC_F32)
    scan_bwd_kernel<float, ORD><<<g, 256, 0, s>>>(a, dy, ld_dy, s0, gi, du, ld_du, dz, ld_dz, ddpre, ld_ddp, slabA,
                                                  slabD, part, o);
  else
    scan_bwd_kernel<bf16_t, ORD><<<g, 256, 0, s>>>(a, dy, ld_dy, s0, gi, du, ld_du, dz, ld_dz, ddpre, ld_ddp, slabA,
                                                   slabD, part, o);
  const long rows = (long)B * L;
  if (dtype == DMC_F32)
    scan_bc_reduce_kernel<float><<<grid_for(rows * (ld_dbc - bc_col)), 256, 0, s>>>(part, rows, G, dbc, ld_dbc, bc_col);
  else
    scan_bc_reduce_kernel<bf16_t><<<grid_for(rows * (ld_dbc - bc_col)), 256, 0, s>>>(part, rows, G, dbc, ld_dbc, bc_col);
  slab_sum_kernel<<<grid_for((long)E * N), 256, 0, s>>>(slabA, B * K, (long)E * N, dA_log);
  slab_sum_kernel<<<grid_for(E), 256, 0, s>>>(slabD, B * K, E, dD);
  return dmc::check_launch(what);
}

}  // namespace

extern "C" int dmc_scan_chunk(void) { return kScanChunk; }

extern "C" int dmc_scan_order_token(int order, int h, int w, int p) {
  if (h <= 0 || w <= 0 || (long)h * w >= (1L << 31) || order < 0 || order > 7 || p < 0 || p >= h * w) return -1;
  return dmc::order_token(dmc::make_scan_ord(h, w, order), p);
}

// The entry points without an order are the ORD = false instantiations: the kernels as they were before the orders.
extern "C" int dmc_causal_conv_silu_fwd(int dtype, const void* x, int ld_x, const float* w, const float* bias, int B,
                                        int L, int E, void* u, int ld_u, void* stream) {
  return conv_fwd_launch<false>("dmc_causal_conv_silu_fwd", dtype, x, ld_x, w, bias, B, L, E, u, ld_u, ScanOrd{},
                                stream);
}

extern "C" int dmc_causal_conv_silu_fwd_ord(int dtype, const void* x, int ld_x, const float* w, const float* bias, int B,
                                            int h, int wt, int order, int E, void* u, int ld_u, void* stream) {
  int L;
  ScanOrd o;
  if (order_check("causal_conv_fwd_ord", h, wt, order, &L, &o)) return 1;
  return conv_fwd_launch<true>("dmc_causal_conv_silu_fwd_ord", dtype, x, ld_x, w, bias, B, L, E, u, ld_u, o, stream);
}

extern "C" size_t dmc_causal_conv_workspace(int B, int L, int E) {
  return (size_t)B * conv_splits(B, L, E) * 5 * E * sizeof(float);
}

extern "C" int dmc_causal_conv_silu_bwd(int dtype, const void* du, int ld_du, const void* x, int ld_x, const float* w,
                                        const float* bias, int B, int L, int E, void* dx, int ld_dx, float* dw,
                                        float* dbias, void* workspace, void* stream) {
  return conv_bwd_launch<false>("dmc_causal_conv_silu_bwd", dtype, du, ld_du, x, ld_x, w, bias, B, L, E, dx, ld_dx, dw,
                                dbias, workspace, ScanOrd{}, stream);
}

extern "C" int dmc_causal_conv_silu_bwd_ord(int dtype, const void* du, int ld_du, const void* x, int ld_x,
                                            const float* w, const float* bias, int B, int h, int wt, int order, int E,
                                            void* dx, int ld_dx, float* dw, float* dbias, void* workspace,
                                            void* stream) {
  int L;
  ScanOrd o;
  if (order_check("causal_conv_bwd_ord", h, wt, order, &L, &o)) return 1;
  return conv_bwd_launch<true>("dmc_causal_conv_silu_bwd_ord", dtype, du, ld_du, x, ld_x, w, bias, B, L, E, dx, ld_dx,
                               dw, dbias, workspace, o, stream);
}

extern "C" size_t dmc_selective_scan_workspace(int B, int L, int E, int N, int backward) {
  const size_t K = (size_t)(L + kScanChunk - 1) / kScanChunk;
  const size_t st = (size_t)B * K * E * N;
  if (!backward) return 2 * st * sizeof(float);
  const size_t G = (size_t)(E + kCB * kBwdSub - 1) / (kCB * kBwdSub);
  return (4 * st + (size_t)B * K * E + (size_t)B * L * G * 2 * N) * sizeof(float);
}

extern "C" int dmc_selective_scan_fwd(int dtype, const void* u, int ld_u, const void* z, int ld_z, const float* dpre,
                                      int ld_dp, const float* Bm, const float* Cm, int ld_bc, const float* A_log,
                                      const float* D, const float* dt_bias, int B, int L, int E, int N, float* states,
                                      void* workspace, void* y, int ld_y, void* stream) {
  return scan_fwd_launch<false>("dmc_selective_scan_fwd", dtype, u, ld_u, z, ld_z, dpre, ld_dp, Bm, Cm, ld_bc, A_log, D,
                                dt_bias, B, L, E, N, states, workspace, y, ld_y, ScanOrd{}, stream);
}

extern "C" int dmc_selective_scan_fwd_ord(int dtype, const void* u, int ld_u, const void* z, int ld_z, const float* dpre,
                                          int ld_dp, const float* Bm, const float* Cm, int ld_bc, const float* A_log,
                                          const float* D, const float* dt_bias, int B, int h, int w, int order, int E,
                                          int N, float* states, void* workspace, void* y, int ld_y, void* stream) {
  int L;
  ScanOrd o;
  if (order_check("selective_scan_fwd_ord", h, w, order, &L, &o)) return 1;
  return scan_fwd_launch<true>("dmc_selective_scan_fwd_ord", dtype, u, ld_u, z, ld_z, dpre, ld_dp, Bm, Cm, ld_bc, A_log,
                               D, dt_bias, B, L, E, N, states, workspace, y, ld_y, o, stream);
}

extern "C" int dmc_selective_scan_bwd(int dtype, const void* dy, int ld_dy, const void* u, int ld_u, const void* z,
                                      int ld_z, const float* dpre, int ld_dp, const float* Bm, const float* Cm, int ld_bc,
                                      const float* A_log, const float* D, const float* dt_bias, int B, int L, int E,
                                      int N, const float* states, void* workspace, void* du, int ld_du, void* dz,
                                      int ld_dz, void* ddpre, int ld_ddp, void* dbc, int ld_dbc, int bc_col,
                                      float* dA_log, float* dD, void* stream) {
  return scan_bwd_launch<false>("dmc_selective_scan_bwd", dtype, dy, ld_dy, u, ld_u, z, ld_z, dpre, ld_dp, Bm, Cm, ld_bc,
                                A_log, D, dt_bias, B, L, E, N, states, workspace, du, ld_du, dz, ld_dz, ddpre, ld_ddp,
                                dbc, ld_dbc, bc_col, dA_log, dD, ScanOrd{}, stream);
}

extern "C" int dmc_selective_scan_bwd_ord(int dtype, const void* dy, int ld_dy, const void* u, int ld_u, const void* z,
                                          int ld_z, const float* dpre, int ld_dp, const float* Bm, const float* Cm,
                                          int ld_bc, const float* A_log, const float* D, const float* dt_bias, int B,
                                          int h, int w, int order, int E, int N, const float* states, void* workspace,
                                          void* du, int ld_du, void* dz, int ld_dz, void* ddpre, int ld_ddp, void* dbc,
                                          int ld_dbc, int bc_col, float* dA_log, float* dD, void* stream) {
  int L;
  ScanOrd o;
  if (order_check("selective_scan_bwd_ord", h, w, order, &L, &o)) return 1;
  return scan_bwd_launch<true>("dmc_selective_scan_bwd_ord", dtype, dy, ld_dy, u, ld_u, z, ld_z, dpre, ld_dp, Bm, Cm,
                               ld_bc, A_log, D, dt_bias, B, L, E, N, states, workspace, du, ld_du, dz, ld_dz, ddpre,
                               ld_ddp, dbc, ld_dbc, bc_col, dA_log, dD, o, stream);
}
