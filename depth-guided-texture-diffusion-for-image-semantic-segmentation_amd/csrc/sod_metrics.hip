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

// one image by one 256-thread block: the LUT, the moments and both curves from its stats and joint histogram into its row `o`
__device__ __forceinline__ void finalize_image(const Stats st, const uint32_t* __restrict__ hist, double* __restrict__ o, int H, int W) {
#pragma clang fp contract(off)
  __shared__ uint32_t fgh[256], bgh[256];
  __shared__ long long ired[4 * 8];
  __shared__ double dred[4 * 10];
  const int t = threadIdx.x;
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

__global__ __launch_bounds__(256) void sodm_finalize_kernel(void* ws, double* __restrict__ out, int H, int W) {
  const int b = blockIdx.x;
  finalize_image(*stats_of(ws, b), hist_of(ws, b), out + (size_t)b * ROW, H, W);
}

// ---- ragged uint8 input: image j is jobs[j].H x jobs[j].W bytes at jobs[j].out_off of pred8 and of gt8 (the packing of
// dgtd_predict_maps: every map starts 16-byte aligned).  blockIdx.y is the job; a lane takes CHUNK = 16 consecutive pixels per step as
// one dwordx4 of each buffer, the last N mod 16 pixels of a map byte by byte (bytes behind a map are never read).  (row, col) comes from
// ONE 32-bit division per chunk (chunk starts are below 2^31) and is stepped from there.
constexpr int CHUNK = 16;
constexpr int RAGGED_MAX_BLOCKS = 32;     // blocks per job: 2 grid-stride steps of 256 lanes x 16 pixels each, up to this many

// the chunk at pixel `base` of an N-pixel map: 16 bytes of each buffer as four words, and how many of them are pixels
__device__ __forceinline__ int load_chunk(const uint8_t* __restrict__ p, const uint8_t* __restrict__ g, uint32_t base, int64_t N, uint32_t (&pw)[4],
                                          uint32_t (&gw)[4]) {
  if ((int64_t)base + CHUNK <= N) {
    const uint4 a = *(const uint4*)(p + base), b = *(const uint4*)(g + base);
    pw[0] = a.x; pw[1] = a.y; pw[2] = a.z; pw[3] = a.w;
    gw[0] = b.x; gw[1] = b.y; gw[2] = b.z; gw[3] = b.w;
    return CHUNK;
  }
  const int n = (int)(N - (int64_t)base);
#pragma unroll
  for (int q = 0; q < 4; ++q) { pw[q] = 0; gw[q] = 0; }
#pragma unroll
  for (int k = 0; k < CHUNK; ++k)
    if (k < n) {
      pw[k >> 2] |= (uint32_t)p[base + k] << (8 * (k & 3));
      gw[k >> 2] |= (uint32_t)g[base + k] << (8 * (k & 3));
    }
  return n;
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[4], int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }

__global__ __launch_bounds__(256) void sodm_ragged_stats_kernel(const uint8_t* __restrict__ pred8, const uint8_t* __restrict__ gt8,
                                                                const dgtd_predict_job* __restrict__ jobs, void* ws) {
  const dgtd_predict_job jb = jobs[blockIdx.y];
  const int W = jb.W;
  const int64_t N = (int64_t)jb.H * W;
  if ((int64_t)blockIdx.x * 256 * CHUNK >= N) return;                        // the whole block lies behind this job's image
  __shared__ uint32_t s_inv_min[4], s_max[4], s_cnt[4];
  __shared__ unsigned long long s_row[4], s_col[4];
  const uint8_t* p = pred8 + jb.out_off;
  const uint8_t* g = gt8 + jb.out_off;
  const int64_t chunks = (N + CHUNK - 1) / CHUNK;
  uint32_t inv_min = 0, mx = 0, cnt = 0;
  unsigned long long srow = 0, scol = 0;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * 256) {
    const uint32_t base = (uint32_t)(c * CHUNK);
    uint32_t pw[4], gw[4];
    const int n = load_chunk(p, g, base, N, pw, gw);
    uint32_t row = base / (uint32_t)W, col = base - row * (uint32_t)W;
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) {
      if (k < n) {
        const uint32_t v = byte_of(pw, k);
        inv_min = max(inv_min, 255u - v);
        mx = max(mx, v);
        if (byte_of(gw, k) > 128u) {
          ++cnt;
          srow += row;
          scol += col;
        }
      }
      if (++col == (uint32_t)W) { col = 0; ++row; }
    }
  }
  // integer reductions (order-free): xor butterfly per wave, the four waves through LDS, one set of global atomics per block
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    inv_min = max(inv_min, (uint32_t)__shfl_xor((int)inv_min, o, 64));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, o, 64));
    cnt += (uint32_t)__shfl_xor((int)cnt, o, 64);
    srow += (unsigned long long)__shfl_xor((long long)srow, o, 64);
    scol += (unsigned long long)__shfl_xor((long long)scol, o, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { s_inv_min[w] = inv_min; s_max[w] = mx; s_cnt[w] = cnt; s_row[w] = srow; s_col[w] = scol; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 4; ++k) {
      inv_min = max(inv_min, s_inv_min[k]);
      mx = max(mx, s_max[k]);
      cnt += s_cnt[k];
      srow += s_row[k];
      scol += s_col[k];
    }
    Stats* st = stats_of(ws, blockIdx.y);
    atomicMax(&st->inv_min, inv_min);
    atomicMax(&st->max, mx);
    if (cnt) { atomicAdd(&st->cnt, cnt); atomicAdd(&st->srow, srow); atomicAdd(&st->scol, scol); }
  }
}

// Joint histogram.  Real saliency maps put most pixels into bins 0 and 255, so one LDS atomic per pixel into one histogram would
// serialise on two addresses.  Two measures: a lane adds a RUN of equal (quadrant, G, p8) keys of its chunk with one atomic (a
// saturated chunk costs one atomic instead of 16), and every wave owns a private copy of the histogram (4 x 8 KiB of LDS), so equal
// keys of different waves never meet.  The copies are summed before the global atomics.
__global__ __launch_bounds__(256) void sodm_ragged_hist_kernel(const uint8_t* __restrict__ pred8, const uint8_t* __restrict__ gt8,
                                                               const dgtd_predict_job* __restrict__ jobs, void* ws) {
  constexpr int BINS = 4 * 2 * 256;
  const dgtd_predict_job jb = jobs[blockIdx.y];
  const int W = jb.W;
  const int64_t N = (int64_t)jb.H * W;
  if ((int64_t)blockIdx.x * 256 * CHUNK >= N) return;
  __shared__ uint32_t h[4 * BINS];
  for (int i = threadIdx.x; i < 4 * BINS; i += 256) h[i] = 0;
  int X, Y;
  split_point(*stats_of(ws, blockIdx.y), &X, &Y);
  __syncthreads();
  uint32_t* mine = h + (threadIdx.x >> 6) * BINS;
  const uint8_t* p = pred8 + jb.out_off;
  const uint8_t* g = gt8 + jb.out_off;
  const int64_t chunks = (N + CHUNK - 1) / CHUNK;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * 256) {
    const uint32_t base = (uint32_t)(c * CHUNK);
    uint32_t pw[4], gw[4];
    const int n = load_chunk(p, g, base, N, pw, gw);
    uint32_t row = base / (uint32_t)W, col = base - row * (uint32_t)W;
    uint32_t run_key = 0, run = 0;
#pragma unroll
    for (int k = 0; k < CHUNK; ++k) {
      if (k < n) {
        const uint32_t q = ((int)row >= Y ? 2u : 0u) + ((int)col >= X ? 1u : 0u);
        const uint32_t key = (q * 2u + (byte_of(gw, k) > 128u ? 1u : 0u)) * 256u + byte_of(pw, k);
        if (key == run_key) {
          ++run;
        } else {
          if (run) atomicAdd(&mine[run_key], run);
          run_key = key;
          run = 1;
        }
      }
      if (++col == (uint32_t)W) { col = 0; ++row; }
    }
    if (run) atomicAdd(&mine[run_key], run);
  }
  __syncthreads();
  uint32_t* gh = hist_of(ws, blockIdx.y);
  for (int i = threadIdx.x; i < BINS; i += 256) {
    const uint32_t v = ((h[i] + h[BINS + i]) + h[2 * BINS + i]) + h[3 * BINS + i];
    if (v) atomicAdd(&gh[i], v);
  }
}

__global__ __launch_bounds__(256) void sodm_ragged_finalize_kernel(const dgtd_predict_job* __restrict__ jobs, void* ws, double* __restrict__ out) {
  const int b = blockIdx.x;
  const dgtd_predict_job jb = jobs[b];
  finalize_image(*stats_of(ws, b), hist_of(ws, b), out + (size_t)b * ROW, jb.H, jb.W);
}

// state += this batch (images in order); slot =(sum sm / n, max(sum em / n), max(sum fm / n))
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

extern "C" int dgtd_sod_metrics_ragged(const uint8_t* pred8, const uint8_t* gt8, int64_t bytes, const dgtd_predict_job* jobs_dev,
                                       const dgtd_predict_job* jobs_host, int njobs, double* out, void* workspace, dgtd_stream s) {
  constexpr int MAX_SIDE = 1 << 24;
  // the job is the grid's second dimension (gridDim.y <= 65535); checked before the table is read
  DGTD_REQUIRE(njobs >= 1 && njobs <= DGTD_PREDICT_MAPS_MAX_JOBS, "sod_metrics_ragged: %d jobs, the grid's second dimension takes 1..%d", njobs,
               DGTD_PREDICT_MAPS_MAX_JOBS);
  DGTD_REQUIRE(pred8 != nullptr && gt8 != nullptr && jobs_dev != nullptr && jobs_host != nullptr && out != nullptr && workspace != nullptr,
               "sod_metrics_ragged: null pointer");
  DGTD_REQUIRE(((uintptr_t)pred8 & 15) == 0 && ((uintptr_t)gt8 & 15) == 0 && ((uintptr_t)jobs_dev & 7) == 0 && ((uintptr_t)workspace & 7) == 0,
               "sod_metrics_ragged: both byte buffers must be 16-byte aligned, the job table and the workspace 8-byte aligned");
  double total = 0.0;
  int64_t max_n = 0;
  for (int j = 0; j < njobs; ++j) {
    const dgtd_predict_job& jb = jobs_host[j];
    DGTD_REQUIRE(jb.H >= 1 && jb.W >= 1 && jb.H <= MAX_SIDE && jb.W <= MAX_SIDE, "sod_metrics_ragged: job %d: bad size H=%d W=%d (sides 1..%d)", j, jb.H,
                 jb.W, MAX_SIDE);
    const int64_t map = (int64_t)jb.H * jb.W;
    DGTD_REQUIRE(map <= (int64_t)1 << 31, "sod_metrics_ragged: job %d: image of %dx%d pixels is too large", j, jb.H, jb.W);
    DGTD_REQUIRE((jb.out_off & 15) == 0, "sod_metrics_ragged: job %d: offset %lld not 16-byte aligned", j, (long long)jb.out_off);
    DGTD_REQUIRE(jb.out_off >= 0 && jb.out_off <= bytes - map, "sod_metrics_ragged: job %d: map [%lld,+%lld) outside the %lld bytes passed in", j,
                 (long long)jb.out_off, (long long)map, (long long)bytes);
    total += (double)map;
    max_n = std::max(max_n, map);
  }
  DGTD_PROF(s, DGTD_HBM, 4.0 * total, "dgtd_sod_metrics_ragged[%d jobs]", njobs);
  hipStream_t st = (hipStream_t)s;
  if (hipMemsetAsync(workspace, 0, (size_t)njobs * WS_IMG, st) != hipSuccess) DGTD_FAIL(3, "sod_metrics_ragged: workspace memset failed");
  const int64_t per_block = (int64_t)2 * 256 * CHUNK;
  const dim3 grid((unsigned)std::min<int64_t>(cdiv(max_n, per_block), RAGGED_MAX_BLOCKS), (unsigned)njobs);
  hipLaunchKernelGGL(sodm_ragged_stats_kernel, grid, dim3(256), 0, st, pred8, gt8, jobs_dev, workspace);
  DGTD_CHECK_LAUNCH("sodm_ragged_stats_kernel");
  hipLaunchKernelGGL(sodm_ragged_hist_kernel, grid, dim3(256), 0, st, pred8, gt8, jobs_dev, workspace);
  DGTD_CHECK_LAUNCH("sodm_ragged_hist_kernel");
  hipLaunchKernelGGL(sodm_ragged_finalize_kernel, dim3(njobs), dim3(256), 0, st, jobs_dev, workspace, out);
  DGTD_CHECK_LAUNCH("sodm_ragged_finalize_kernel");
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
