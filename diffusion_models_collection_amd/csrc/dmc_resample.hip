// Loss-aware timestep sampling (Nichol & Dhariwal 2021, arXiv:2102.09672 §3.3), device-resident (gfx950). Not in the
// reference. The history of the last K losses per timestep, its counts, the probabilities, the CDF, the draw and the
// importance weights stay in HBM: one launch after the loss (ts_history_update_kernel), one before the next forward
// (ts_sample_kernel), nothing read back, no atomics, no RNG.
//
// Compiled with -ffp-contract=off: the double arithmetic of ts_sample_kernel is one rounding per op, as the host
// restatement (diffusion/_resample.py) has it.
#include "dmc_common.h"
#include "dmc_internal.h"

#define DMC_TS_CHUNK 1024   // batch entries staged in LDS per pass of ts_history_update_kernel

namespace {

DMC_DEV int ts_clamp(long t, int T) { return (int)(t < 0 ? 0 : (t > T - 1 ? T - 1 : t)); }   // never index past a row

// One thread per timestep; the batch goes through LDS in chunks of DMC_TS_CHUNK and every thread scans it in index
// order (all lanes read the same entry: a broadcast), taking the entries of its own timestep. Row tt is written by its
// thread alone, in the sequential loop's order, whatever the duplicates in the batch: no atomics, deterministic.
__global__ __launch_bounds__(256) void ts_history_update_kernel(const int64_t* t, const float* loss, int N, int T, int K,
                                                                float* hist, int32_t* count) {
  __shared__ int st[DMC_TS_CHUNK];
  __shared__ float sl[DMC_TS_CHUNK];
  const int tt = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = tt < T;
  int c = live ? count[tt] : 0;
  int slot = (int)((unsigned)c % (unsigned)K);   // in [0, K) for any bit pattern of c
  float* row = hist + (size_t)(live ? tt : 0) * K;
  for (int n0 = 0; n0 < N; n0 += DMC_TS_CHUNK) {
    const int cnt = N - n0 < DMC_TS_CHUNK ? N - n0 : DMC_TS_CHUNK;
    for (int j = threadIdx.x; j < cnt; j += blockDim.x) {
      st[j] = ts_clamp(t[n0 + j], T);
      sl[j] = loss[n0 + j];
    }
    __syncthreads();
    if (live) {
      for (int j = 0; j < cnt; ++j) {
        if (st[j] == tt) {
          row[slot] = sl[j];
          if (++slot == K) slot = 0;
          ++c;
        }
      }
    }
    __syncthreads();   // the next chunk overwrites st / sl
  }
  if (live) count[tt] = c;
}

// sum over the block of v, the same value in every thread: a fixed tree over thread indices
DMC_DEV double ts_block_sum(double v, double* sm) {
  sm[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sm[threadIdx.x] += sm[threadIdx.x + s];
    __syncthreads();
  }
  const double r = sm[0];
  __syncthreads();   // sm is reused
  return r;
}

// r_t = sqrt(mean_k hist[t][k]^2), k in index order
DMC_DEV double ts_rms(const float* hist, int t, int K) {
  const float* row = hist + (size_t)t * K;
  double a = 0.0;
  for (int k = 0; k < K; ++k) {
    const double h = (double)row[k];
    a += h * h;
  }
  return sqrt(a / (double)K);
}

// One block of 256 threads, tiles of 256 timesteps in index order (thread i of a tile owns timestep base + i). r_t is
// recomputed in each of the three passes (K loads from a row that stays in cache) instead of kept, so any T works.
// Thread i's partial sums take its timesteps in ascending order and ts_block_sum's tree is fixed: the same bits on every
// run. The scan is Hillis-Steele per tile in double, plus the carry of the tiles before.
__global__ __launch_bounds__(256) void ts_sample_kernel(const float* hist, const int32_t* count, int T, int K,
                                                        float uniform_prob, const float* u, int N, int64_t* t_out,
                                                        float* p, float* iw, float* cdf) {
  __shared__ double sm[256];
  __shared__ int cold;
  const int tid = threadIdx.x;
  if (tid == 0) cold = 0;
  __syncthreads();
  bool mine_cold = false;
  double s = 0.0;
  for (int i = tid; i < T; i += 256) {
    if (count[i] < K) mine_cold = true;
    s += ts_rms(hist, i, K);
  }
  if (mine_cold) cold = 1;   // every writer stores the same value
  const double S = ts_block_sum(s, sm);   // its barriers order the flag as well
  const double dT = (double)T, up = (double)uniform_prob;
  const bool uniform = cold != 0 || !(S > 0.0 && S <= 1.7976931348623157e308);   // NaN fails S > 0
  double Q = 1.0;
  if (!uniform) {
    double q = 0.0;
    for (int i = tid; i < T; i += 256) q += ts_rms(hist, i, K) / S * (1.0 - up) + up / dT;
    Q = ts_block_sum(q, sm);
  }
  double carry = 0.0;
  for (int base = 0; base < T; base += 256) {
    const int i = base + tid;
    double pi = 0.0;
    if (i < T) {
      if (uniform) {
        p[i] = (float)(1.0 / dT);
        iw[i] = 1.f;
      } else {
        pi = (ts_rms(hist, i, K) / S * (1.0 - up) + up / dT) / Q;
        p[i] = (float)pi;
        iw[i] = (float)(1.0 / (dT * pi));
      }
    }
    if (uniform) {
      if (i < T) cdf[i] = i == T - 1 ? 1.f : (float)((double)(i + 1) / dT);
      continue;
    }
    sm[tid] = pi;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {
      const double add = tid >= o ? sm[tid - o] : 0.0;
      __syncthreads();
      sm[tid] += add;
      __syncthreads();
    }
    if (i < T) cdf[i] = i == T - 1 ? 1.f : (float)(carry + sm[tid]);
    carry += sm[255];
    __syncthreads();   // sm is rewritten by the next tile
  }
  __syncthreads();   // the block's cdf stores are visible to its own loads below
  for (int n = tid; n < N; n += 256) {
    const float un = u[n];
    int lo = 0, hi = T - 1;   // the smallest i with cdf[i] > u; T - 1 when none is (u >= 1 or NaN)
    while (lo < hi) {
      const int mid = lo + (hi - lo) / 2;
      if (cdf[mid] > un) hi = mid;
      else lo = mid + 1;
    }
    t_out[n] = lo;
  }
}

}  // namespace

extern "C" int dmc_ts_history_update(const int64_t* t, const float* loss, int N, int T, int K, float* hist,
                                     int32_t* count, void* stream) {
  DMC_REQUIRE(N > 0 && T > 0 && K > 0, "ts_history_update: N %d, T %d, K %d must be positive", N, T, K);
  DMC_REQUIRE(t && loss && hist && count, "ts_history_update: t, loss, hist and count must not be NULL");
  ts_history_update_kernel<<<dmc::cdiv(T, 256), 256, 0, dmc::as_stream(stream)>>>(t, loss, N, T, K, hist, count);
  return dmc::check_launch("dmc_ts_history_update");
}

extern "C" int dmc_ts_sample(const float* hist, const int32_t* count, int T, int K, float uniform_prob, const float* u,
                             int N, int64_t* t_out, float* p, float* iw, float* cdf, void* stream) {
  DMC_REQUIRE(N > 0 && T > 0 && K > 0, "ts_sample: N %d, T %d, K %d must be positive", N, T, K);
  DMC_REQUIRE(uniform_prob >= 0.f && uniform_prob < 1.f, "ts_sample: uniform_prob %g is not in [0, 1)",
              (double)uniform_prob);
  DMC_REQUIRE(hist && count && u && t_out && p && iw && cdf,
              "ts_sample: hist, count, u, t_out, p, iw and cdf must not be NULL");
  ts_sample_kernel<<<1, 256, 0, dmc::as_stream(stream)>>>(hist, count, T, K, uniform_prob, u, N, t_out, p, iw, cdf);
  return dmc::check_launch("dmc_ts_sample");
}
