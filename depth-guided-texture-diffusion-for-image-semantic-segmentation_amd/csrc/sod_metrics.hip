// sod_metrics.hip — S-measure, E-measure, F-measure and MAE of py_sod_metrics 1.3.1 (as twig/metric/{S,E,F}measure.py and MAE.py
// call it) on the device, for the validation loop.  Both maps are quantised to uint8 by the wrappers, so every fp64 quantity of the
// package is a function of (p8, gt > 128, quadrant): integer histograms carry all the data and the fp64 work is 256 entries per image.
//   1. stats     (tiles x images): min/max of p8, count(G), sum of row / column of the G pixels        (integer atomics: exact)
//   2. histogram (tiles x images): joint [quadrant 4][G 2][p8 256] histogram about the rounded centroid (LDS, then integer atomics)
//   3. finalise  (one block per image, fp64): the LUT P(t) in NumPy's operation order, count-weighted moments, both curves
//   4. accumulate (one block): running sums over every image seen, and the wrappers' running (sm, max em, max fm) triple
// Integer work is order-free; fp64 reductions run in a fixed order, so two runs are bit-identical.  No FMA contraction anywhere the
// quantisation or the fp64 metric arithmetic happens (the build uses -ffp-contract=fast; one fused multiply-add moves a uint8 bin).
#include "common.h"

namespace {

constexpr int ROW = DGTD_SODM_ROW;        // doubles per image of `out`
constexpr int STATE = DGTD_SODM_STATE;    // doubles of the running state
constexpr size_t WS_IMG = 32 + 4 * 2 * 256 * 4;  // per image: stats (u32 inv_min, max, cnt, pad; u64 srow, scol) + joint histogram
constexpr double EPS = 2.220446049250313e-16;    // np.spacing(1)
constexpr double BETA = 0.3;                     // F-measure beta^2

struct Stats { uint32_t inv_min, max, cnt, pad; unsigned long long srow, scol; };

__device__ __forceinline__ Stats* stats_of(void* ws, int b) { return (Stats*)((char*)ws + (size_t)b * WS_IMG); }
__device__ __forceinline__ uint32_t* hist_of(void* ws, int b) { return (uint32_t*)((char*)ws + (size_t)b * WS_IMG + 32); }

// wrapper quantisation (twig/metric/*measure.py: (x * 255).astype(np.uint8)): fp32 multiply, truncation.  Sigmoid outputs are in
// [0, 1]; anything outside (where NumPy's cast is undefined) is clamped.
__device__ __forceinline__ int quant8(float v) {
#pragma clang fp contract(off)
  const float s = v * 255.0f;
  if (!(s > 0.0f)) return 0;
  if (s >= 255.0f) return 255;
  return (int)s;
}

// (X, Y) = int(round(centroid)) + 1 of the G pixels (round half to even); unused unless 0 < count(G) < N
__device__ __forceinline__ void split_point(const Stats& s, int* X, int* Y) {
#pragma clang fp contract(off)
  if (s.cnt == 0) { *X = 0; *Y = 0; return; }
  *Y = (int)rint((double)s.srow / (double)s.cnt) + 1;
  *X = (int)rint((double)s.scol / (double)s.cnt) + 1;
}

template <typename T>
__global__ __launch_bounds__(256) void sodm_stats_kernel(const T* __restrict__ pred, const float* __restrict__ gt, void* ws, int H, int W) {
  __shared__ uint32_t s_inv_min, s_max, s_cnt;
  __shared__ unsigned long long s_row, s_col;
  if (threadIdx.x == 0) { s_inv_min = 0; s_max = 0; s_cnt = 0; s_row = 0; s_col = 0; }
  __syncthreads();
  const int b = blockIdx.y;
  const int64_t N = (int64_t)H * W;
  const T* p = pred + (size_t)b * N;
  const float* g = gt + (size_t)b * N;
  uint32_t inv_min = 0, mx = 0, cnt = 0;
  unsigned long long srow = 0, scol = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const uint32_t v = (uint32_t)quant8(to_f(p[i]));
    inv_min = max(inv_min, 255u - v);
    mx = max(mx, v);
    if (quant8(g[i]) > 128) {
      ++cnt;
      srow += (unsigned long long)(i / W);
      scol += (unsigned long long)(i % W);
    }
  }
  atomicMax(&s_inv_min, inv_min);
  atomicMax(&s_max, mx);
  if (cnt) { atomicAdd(&s_cnt, cnt); atomicAdd(&s_row, srow); atomicAdd(&s_col, scol); }
  __syncthreads();
  if (threadIdx.x == 0) {
    Stats* st = stats_of(ws, b);
    atomicMax(&st->inv_min, s_inv_min);
    atomicMax(&st->max, s_max);
    if (s_cnt) { atomicAdd(&st->cnt, s_cnt); atomicAdd(&st->srow, s_row); atomicAdd(&st->scol, s_col); }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void sodm_hist_kernel(const T* __restrict__ pred, const float* __restrict__ gt, void* ws, int H, int W) {
  __shared__ uint32_t h[4 * 2 * 256];
  for (int i = threadIdx.x; i < 4 * 2 * 256; i += 256) h[i] = 0;
  const int b = blockIdx.y;
  int X, Y;
  split_point(*stats_of(ws, b), &X, &Y);
  __syncthreads();
  const int64_t N = (int64_t)H * W;
  const T* p = pred + (size_t)b * N;
  const float* g = gt + (size_t)b * N;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < N; i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i / W), c = (int)(i % W);
    const int q = (r >= Y ? 2 : 0) + (c >= X ? 1 : 0);
    const int gb = quant8(g[i]) > 128 ? 1 : 0;
    atomicAdd(&h[(q * 2 + gb) * 256 + quant8(to_f(p[i]))], 1u);
  }
  __syncthreads();
  uint32_t* gh = hist_of(ws, b);
  for (int i = threadIdx.x; i < 4 * 2 * 256; i += 256)
    if (h[i]) atomicAdd(&gh[i], h[i]);
}

// sum of K values over the 256-thread block in a fixed order (xor butterfly per wave, then waves 0..3); every thread gets the result
template <typename V, int K>
__device__ __forceinline__ void block_sum(V (&v)[K], V* red /* LDS [4 * K] */) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k)
    for (int o = 32; o > 0; o >>= 1) v[k] = v[k] + __shfl_xor(v[k], o, 64);
  if (lane == 0)
    for (int k = 0; k < K; ++k) red[w * K + k] = v[k];
  __syncthreads();
  for (int k = 0; k < K; ++k) v[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
  __syncthreads();
}

// Emeasure.cal_em_with_threshold / cal_em_with_cumsumhistogram for one threshold (Emeasure.py:137-243): the two degenerate gt
// branches, generate_parts_numel_combinations, parts summed 0+1+2+3, / (N - 1 + EPS)
__device__ double em_value(long long fgfg, long long fgbg, long long gfg, long long N) {
#pragma clang fp contract(off)
  const long long fg = fgfg + fgbg, bg = N - fg;
  double sum;
  if (gfg == 0) {
    sum = (double)bg;
  } else if (gfg == N) {
    sum = (double)fg;
  } else {
    const long long bgfg = gfg - fgfg, bgbg = bg - bgfg;
    const double mp = (double)fg / (double)N, mg = (double)gfg / (double)N;
    const double pf = 1.0 - mp, pb = 0.0 - mp, gf = 1.0 - mg, gb = 0.0 - mg;
    const double a[4] = {pf, pf, pb, pb}, c[4] = {gf, gb, gf, gb};
    const long long n[4] = {fgfg, fgbg, bgfg, bgbg};
    sum = 0.0;
    for (int i = 0; i < 4; ++i) {
      const double align = 2.0 * (a[i] * c[i]) / ((a[i] * a[i] + c[i] * c[i]) + EPS);
      const double e = (align + 1.0) * (align + 1.0) / 4.0;
      sum = sum + e * (double)n[i];
    }
  }
  return sum / ((double)(N - 1) + EPS);
}

// 2 * mean / (mean^2 + 1 + std + EPS)  (Smeasure.s_object)
__device__ __forceinline__ double s_object(double m, double sd) {
#pragma clang fp contract(off)
  return 2.0 * m / (((m * m + 1.0) + sd) + EPS);
}

__global__ __launch_bounds__(256) void sodm_finalize_kernel(void* ws, double* __restrict__ out, int H, int W) {
#pragma clang fp contract(off)
  __shared__ uint32_t fgh[256], bgh[256];
  __shared__ long long ired[4 * 8];
  __shared__ double dred[4 * 10];
  const int b = blockIdx.x, t = threadIdx.x;
  const Stats st = *stats_of(ws, b);
  const uint32_t* hist = hist_of(ws, b);
  const long long N = (long long)H * W, cnt = st.cnt;
  fgh[t] = 0;
  bgh[t] = 0;
  long long c0q[4], c1q[4];
  long long c0 = 0, c1 = 0;
  for (int q = 0; q < 4; ++q) {
    c0q[q] = hist[(q * 2 + 0) * 256 + t];
    c1q[q] = hist[(q * 2 + 1) * 256 + t];
    c0 += c0q[q];
    c1 += c1q[q];
  }
  const bool have = (c0 + c1) > 0;
  // _prepare_data: P = p8 / 255, min-max normalised when max != min
  const int mn = 255 - (int)st.inv_min, mx = (int)st.max;
  double P = (double)t / 255.0;
  if (mx != mn) P = (P - (double)mn / 255.0) / ((double)mx / 255.0 - (double)mn / 255.0);
  __syncthreads();
  if (have) {                                            // second quantisation of the curves: (P * 255).astype(np.uint8)
    int qb = (int)(P * 255.0);
    qb = qb < 0 ? 0 : (qb > 255 ? 255 : qb);
    atomicAdd(&fgh[qb], (uint32_t)c1);
    atomicAdd(&bgh[qb], (uint32_t)c0);
  }
  // integer sums: pixels and G pixels per quadrant
  long long nq[8];
  for (int q = 0; q < 4; ++q) { nq[q] = c0q[q] + c1q[q]; nq[4 + q] = c1q[q]; }
  block_sum(nq, ired);
  // first fp64 moments: sum P, sum |P - G|, sum P over G, sum (1 - P) over ~G, sum P per quadrant
  double m1[8];
  m1[0] = have ? (double)(c0 + c1) * P : 0.0;
  m1[1] = have ? (double)c0 * fabs(P) + (double)c1 * fabs(P - 1.0) : 0.0;
  m1[2] = c1 ? (double)c1 * P : 0.0;
  m1[3] = c0 ? (double)c0 * (1.0 - P) : 0.0;
  for (int q = 0; q < 4; ++q) m1[4 + q] = (c0q[q] + c1q[q]) ? (double)(c0q[q] + c1q[q]) * P : 0.0;
  block_sum(m1, dred);
  const double mean = m1[0] / (double)N;
  const double thr = 1.0 < 2.0 * mean ? 1.0 : 2.0 * mean;     // min(2 * P.mean(), 1)
  const double mfg = m1[2] / (double)cnt, mbg = m1[3] / (double)(N - cnt);
  double xq[4], yq[4];
  for (int q = 0; q < 4; ++q) { xq[q] = m1[4 + q] / (double)nq[q]; yq[q] = (double)nq[4 + q] / (double)nq[q]; }
  // adaptive threshold: binarised P >= thr over G and over ~G
  long long ad[2] = {have && P >= thr ? c1 : 0, have && P >= thr ? c0 : 0};
  block_sum(ad, ired);
  // second fp64 moments (two-pass, mean first, as NumPy's std / the ssim sums)
  double m2[10];
  m2[0] = c1 ? (double)c1 * ((P - mfg) * (P - mfg)) : 0.0;
  m2[1] = c0 ? (double)c0 * (((1.0 - P) - mbg) * ((1.0 - P) - mbg)) : 0.0;
  for (int q = 0; q < 4; ++q) {
    const long long n = c0q[q] + c1q[q];
    const double dx = P - xq[q];
    m2[2 + q] = n ? (double)n * (dx * dx) : 0.0;
    m2[6 + q] = n ? (double)c1q[q] * (dx * (1.0 - yq[q])) + (double)c0q[q] * (dx * (0.0 - yq[q])) : 0.0;
  }
  block_sum(m2, dred);

  // curves: index i <-> threshold 255 - i (cumsum of the flipped histograms)
  long long tp = 0, fp = 0;
  for (int k = 255 - t; k < 256; ++k) { tp += fgh[k]; fp += bgh[k]; }
  double* o = out + (size_t)b * ROW;
  {
    long long ps = tp + fp;
    if (ps == 0) ps = 1;
    const long long T = cnt > 0 ? cnt : 1;
    const double prec = (double)tp / (double)ps, rec = (double)tp / (double)T;
    const double num = (1.0 + BETA) * prec * rec;
    const double den = num == 0.0 ? 1.0 : BETA * prec + rec;
    o[4 + t] = em_value(tp, fp, cnt, N);
    o[260 + t] = num / den;
    o[516 + t] = prec;
    o[772 + t] = rec;
  }
  if (t == 0) {
    const double mae = m1[1] / (double)N;
    // adaptive F-measure
    double adp_fm = 0.0;
    if (ad[0] != 0) {
      const double pre = (double)ad[0] / (double)(ad[0] + ad[1]), rec = (double)ad[0] / (double)cnt;
      adp_fm = (1.0 + BETA) * pre * rec / (BETA * pre + rec);
    }
    const double adp_em = em_value(ad[0], ad[1], cnt, N);
    // S-measure (alpha = 0.5)
    double sm;
    if (cnt == 0) {
      sm = 1.0 - mean;
    } else if (cnt == N) {
      sm = mean;
    } else {
      const double u = (double)cnt / (double)N;
      const double sd_fg = sqrt(m2[0] / (double)(cnt - 1)), sd_bg = sqrt(m2[1] / (double)(N - cnt - 1));
      const double object = u * s_object(mfg, sd_fg) + (1.0 - u) * s_object(mbg, sd_bg);
      int X, Y;
      split_point(st, &X, &Y);
      const double w1 = (double)((long long)X * Y) / (double)N;
      const double w2 = (double)((long long)Y * (W - X)) / (double)N;
      const double w3 = (double)((long long)(H - Y) * X) / (double)N;
      const double wq[4] = {w1, w2, w3, ((1.0 - w1) - w2) - w3};
      double region = 0.0;
      for (int q = 0; q < 4; ++q) {
        const double n1 = (double)(nq[q] - 1), x = xq[q], y = yq[q];
        const double sx = m2[2 + q] / n1;
        const double sy = ((double)nq[4 + q] * ((1.0 - y) * (1.0 - y)) + (double)(nq[q] - nq[4 + q]) * ((0.0 - y) * (0.0 - y))) / n1;
        const double sxy = m2[6 + q] / n1;
        const double alpha = 4.0 * x * y * sxy;
        const double beta = (x * x + y * y) * (sx + sy);
        const double score = alpha != 0.0 ? alpha / (beta + EPS) : (beta == 0.0 ? 1.0 : 0.0);
        region = q == 0 ? wq[0] * score : region + wq[q] * score;
      }
      sm = 0.5 * object + 0.5 * region;
      sm = sm > 0.0 ? sm : 0.0;                          // Python max(0, sm): NaN reports 0
    }
    o[0] = mae;
    o[1] = sm;
    o[2] = adp_em;
    o[3] = adp_fm;
  }
}

// state += this batch (images in order); slot = (sum sm / n, max(sum em / n), max(sum fm / n))
__global__ __launch_bounds__(256) void sodm_accumulate_kernel(const double* __restrict__ out, int B, double* __restrict__ state,
                                                              double* __restrict__ slot) {
#pragma clang fp contract(off)
  __shared__ double red[2 * 4];
  const int t = threadIdx.x;
  const double n = state[0] + (double)B;
  double se = state[8 + t], sf = state[264 + t];
  for (int b = 0; b < B; ++b) {
    se = se + out[(size_t)b * ROW + 4 + t];
    sf = sf + out[(size_t)b * ROW + 260 + t];
  }
  state[8 + t] = se;
  state[264 + t] = sf;
  double em = se / n, fm = sf / n;
  for (int o = 32; o > 0; o >>= 1) {
    const double e2 = __shfl_xor(em, o, 64), f2 = __shfl_xor(fm, o, 64);
    em = e2 > em ? e2 : em;
    fm = f2 > fm ? f2 : fm;
  }
  if ((t & 63) == 0) { red[(t >> 6) * 2] = em; red[(t >> 6) * 2 + 1] = fm; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 4; ++w) {
      em = red[w * 2] > em ? red[w * 2] : em;
      fm = red[w * 2 + 1] > fm ? red[w * 2 + 1] : fm;
    }
    double s[4] = {state[1], state[2], state[3], state[4]};
    for (int b = 0; b < B; ++b)
      for (int k = 0; k < 4; ++k) s[k] = s[k] + out[(size_t)b * ROW + (k == 0 ? 1 : k == 1 ? 0 : k)];
    state[0] = n;
    for (int k = 0; k < 4; ++k) state[1 + k] = s[k];
    slot[0] = s[0] / n;
    slot[1] = em;
    slot[2] = fm;
  }
}

}  // namespace

extern "C" int64_t dgtd_sod_metrics_workspace(int B) { return B > 0 ? (int64_t)B * (int64_t)WS_IMG : 0; }

extern "C" int dgtd_sod_metrics(const void* pred, dgtd_dtype pred_dt, const float* gt, double* out, void* workspace, int B, int H, int W,
                                dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, (double)B * H * W * (2.0 * dgtd_esize(pred_dt) + 8.0), "dgtd_sod_metrics[B=%d,%dx%d]", B, H, W);
  DGTD_REQUIRE(B > 0 && H > 0 && W > 0, "sod_metrics: bad sizes B=%d H=%d W=%d", B, H, W);
  DGTD_REQUIRE((int64_t)H * W <= (int64_t)1 << 31, "sod_metrics: image of %dx%d pixels is too large", H, W);
  DGTD_REQUIRE(pred_dt == DGTD_F32 || DGTD_IS_HALF(pred_dt), "sod_metrics: bad pred dtype %d", (int)pred_dt);
  DGTD_REQUIRE(pred && gt && out && workspace, "sod_metrics: null pointer");
  hipStream_t st = (hipStream_t)s;
  if (hipMemsetAsync(workspace, 0, (size_t)B * WS_IMG, st) != hipSuccess) DGTD_FAIL(3, "sod_metrics: workspace memset failed");
  const int64_t N = (int64_t)H * W;
  const dim3 grid((unsigned)(cdiv(N, 8192) < 16 ? cdiv(N, 8192) : 16), (unsigned)B);
  DGTD_DISPATCH(pred_dt, hipLaunchKernelGGL(sodm_stats_kernel<T_>, grid, dim3(256), 0, st, (const T_*)pred, gt, workspace, H, W));
  DGTD_CHECK_LAUNCH("sodm_stats_kernel");
  DGTD_DISPATCH(pred_dt, hipLaunchKernelGGL(sodm_hist_kernel<T_>, grid, dim3(256), 0, st, (const T_*)pred, gt, workspace, H, W));
  DGTD_CHECK_LAUNCH("sodm_hist_kernel");
  hipLaunchKernelGGL(sodm_finalize_kernel, dim3(B), dim3(256), 0, st, workspace, out, H, W);
  DGTD_CHECK_LAUNCH("sodm_finalize_kernel");
  return 0;
}

extern "C" int dgtd_sod_metrics_accumulate(const double* out, int B, double* state, double* running_slot, dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, (double)B * ROW * 8.0 + 2.0 * STATE * 8.0, "dgtd_sod_metrics_accumulate[B=%d]", B);
  DGTD_REQUIRE(B > 0, "sod_metrics_accumulate: bad batch %d", B);
  DGTD_REQUIRE(out && state && running_slot, "sod_metrics_accumulate: null pointer");
  hipLaunchKernelGGL(sodm_accumulate_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, out, B, state, running_slot);
  DGTD_CHECK_LAUNCH("sodm_accumulate_kernel");
  return 0;
}
