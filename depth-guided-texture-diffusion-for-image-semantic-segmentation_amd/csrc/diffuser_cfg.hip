// diffuser_cfg.hip — the texture diffuser front end with RUNTIME grid G, neighbourhood K, step count and latent width
// (fwd + bwd, fp32 throughout).  diffuser.hip keeps the reference configuration (12, 7, 4, 24) as compile-time constants with its
// 49x144 weights in LDS; this family covers 2 <= G <= 64, odd 3 <= K <= 11, 0 <= steps <= 64, 1 <= LAT <= 64, where the
// normalised weights reach K^2 G^2 4 B = 2 MB per (image, channel) and fit no LDS.
//
// Where things live (one workgroup per (image, channel), cells looped over by the threads):
//   * normalised weights Wn[K^2][G^2] and 1/(sum + eps): caller's workspace (global, L2-resident for small grids).  Thread p writes and,
//     in the forward, reads only column p, so the forward needs no barrier between the regressor and the first step;
//   * the propagating state: two G^2 buffers in LDS (<= 32 KB), ping-pong, one barrier per step;
//   * backward only: every state x_s and every back-propagated gradient g_{s+1} in the workspace; the per-tap accumulator
//     dWn[t][p] = sum_s g_{s+1}[p] x_s[p + off(t)] is then formed per (t, p) in registers and overwrites Wn[t][p] in place (first
//     as dWn, then as dz), so no second K^2 G^2 buffer exists.
// Same index rules as diffuser.hip (PyTorch nearest / bilinear, align_corners=False); nothing assumes S >= G.
#include "common.h"

namespace {

constexpr int MAXG = 64, MAXP = MAXG * MAXG, MAXK = 11, MAXSTEPS = 64, MAXLAT = 64, MAXWAVES = 16;

struct Cfg { int S, G, P, K, T, steps, LAT; };

__device__ __forceinline__ int nearest_src(int dst, float scale, int in) { return min((int)floorf(dst * scale), in - 1); }
__device__ __forceinline__ void bilinear_src(int dst, float scale, int in, int& i0, int& i1, float& l1) {
  float src = scale * (dst + 0.5f) - 0.5f;
  if (src < 0.f) src = 0.f;
  i0 = min((int)src, in - 1);
  i1 = i0 + ((i0 < in - 1) ? 1 : 0);
  l1 = src - (float)i0;
}
__device__ __forceinline__ float sigmoidf(float z) { return 1.f / (1.f + expf(-z)); }

// sum over the workgroup (<= 16 waves), the same fixed order in every thread; `red` holds MAXWAVES floats
__device__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int nw = (blockDim.x + 63) >> 6;
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = 0.f;
  for (int i = 0; i < nw; ++i) s += red[i];
  __syncthreads();
  return s;
}

// per-(image, channel) slices of the workspace, in floats
__host__ __device__ inline size_t ws_fwd_floats(int P, int T) { return (size_t)(T + 1) * P; }
__host__ __device__ inline size_t ws_bwd_floats(int P, int T, int steps) { return (size_t)(T + 1) * P + 2 * (size_t)steps * P; }

__device__ __forceinline__ void hp_sample(const Cfg& q, const float* __restrict__ x_hp, int b, int p, float x[3]) {
  const float scale = (float)q.S / (float)q.G;
  const int sy = nearest_src(p / q.G, scale, q.S), sx = nearest_src(p % q.G, scale, q.S);
#pragma unroll
  for (int i = 0; i < 3; ++i) x[i] = x_hp[(((size_t)b * 3 + i) * q.S + sy) * q.S + sx];
}
__device__ __forceinline__ float depth_sample(const Cfg& q, const float* __restrict__ depth, int b, int p) {
  const float scale = (float)q.S / (float)q.G;
  int y0, y1, x0, x1; float ly, lx;
  bilinear_src(p / q.G, scale, q.S, y0, y1, ly);
  bilinear_src(p % q.G, scale, q.S, x0, x1, lx);
  const float* d = depth + (size_t)b * q.S * q.S;
  return (1.f - ly) * ((1.f - lx) * d[(size_t)y0 * q.S + x0] + lx * d[(size_t)y0 * q.S + x1]) +
         ly * ((1.f - lx) * d[(size_t)y1 * q.S + x0] + lx * d[(size_t)y1 * q.S + x1]);
}

// Shared forward body.  Fills Wn / inv (when steps > 0), leaves the final state in lds[(steps & 1) * P ...]; with `st` non-null also
// writes the states x_0 .. x_{steps-1} there.  Wn, inv, st alias the caller's workspace: no __restrict__.
__device__ void forward_body(const Cfg& q, float* lds, const float* __restrict__ x_hp, const float* __restrict__ depth,
                             const float* __restrict__ reg_w, const float* __restrict__ reg_b, const float* __restrict__ enc_w,
                             const float* __restrict__ enc_b, float* Wn, float* inv, float* st, int b, int c) {
  const int P = q.P, T = q.T, G = q.G, K = q.K, R = K / 2;
  for (int p = threadIdx.x; p < P; p += blockDim.x) {
    const float x0 = enc_w[c] * depth_sample(q, depth, b, p) + enc_b[c];
    lds[p] = x0;
    if (st != nullptr && q.steps > 0) st[p] = x0;
    if (q.steps > 0) {
      float x[3];
      hp_sample(q, x_hp, b, p, x);
      // two passes over the taps, the sigmoid evaluated in both: 2 K^2 exponentials per cell are cheaper than writing the raw weights
      // and scaling them in place (for the large grids the weights stream through HBM)
      float sum = 0.f;
      for (int t = 0; t < T; ++t) {
        const float* w = reg_w + (size_t)(c * T + t) * 3;
        sum += sigmoidf(w[0] * x[0] + w[1] * x[1] + w[2] * x[2] + reg_b[c * T + t]);
      }
      const float iv = 1.f / (sum + 1e-5f);   // taken over all K^2 taps: border weights are not renormalised
      inv[p] = iv;
      for (int t = 0; t < T; ++t) {
        const float* w = reg_w + (size_t)(c * T + t) * 3;
        Wn[(size_t)t * P + p] = sigmoidf(w[0] * x[0] + w[1] * x[1] + w[2] * x[2] + reg_b[c * T + t]) * iv;
      }
    }
  }
  __syncthreads();
  for (int step = 0; step < q.steps; ++step) {
    const float* src = lds + (step & 1) * P;
    float* dst = lds + ((step + 1) & 1) * P;
    for (int p = threadIdx.x; p < P; p += blockDim.x) {
      const int py = p / G, px = p % G;
      float acc = 0.f;
      for (int ky = 0; ky < K; ++ky) {
        const int yy = py + ky - R;
        if (yy < 0 || yy >= G) continue;
        for (int kx = 0; kx < K; ++kx) {
          const int xq = px + kx - R;
          if (xq < 0 || xq >= G) continue;
          acc += Wn[(size_t)(ky * K + kx) * P + p] * src[yy * G + xq];
        }
      }
      dst[p] = acc;
      if (st != nullptr && step + 1 < q.steps) st[(size_t)(step + 1) * P + p] = acc;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(1024) void diffuser_cfg_fwd_kernel(const float* __restrict__ x_hp, const float* __restrict__ depth,
                                                                const float* __restrict__ reg_w, const float* __restrict__ reg_b,
                                                                const float* __restrict__ enc_w, const float* __restrict__ enc_b,
                                                                float* __restrict__ x4, float* ws, Cfg q) {
  __shared__ float lds[2 * MAXP];
  const int c = blockIdx.x, b = blockIdx.y;
  float* Wn = ws + ((size_t)b * q.LAT + c) * ws_fwd_floats(q.P, q.T);
  forward_body(q, lds, x_hp, depth, reg_w, reg_b, enc_w, enc_b, Wn, Wn + (size_t)q.T * q.P, nullptr, b, c);
  const float* fin = lds + (q.steps & 1) * q.P;
  for (int p = threadIdx.x; p < q.P; p += blockDim.x) x4[((size_t)b * q.LAT + c) * q.P + p] = fin[p];
}

// backward w.r.t. the parameters (inputs carry no gradient).  d_* are accumulated with atomics over the batch (zeroed by the caller).
__global__ __launch_bounds__(1024) void diffuser_cfg_bwd_kernel(const float* __restrict__ x_hp, const float* __restrict__ depth,
                                                                const float* __restrict__ reg_w, const float* __restrict__ reg_b,
                                                                const float* __restrict__ enc_w, const float* __restrict__ enc_b,
                                                                const float* __restrict__ g4, float* __restrict__ d_reg_w,
                                                                float* __restrict__ d_reg_b, float* __restrict__ d_enc_w,
                                                                float* __restrict__ d_enc_b, float* ws, Cfg q) {
  __shared__ float lds[3 * MAXP];
  __shared__ float red[MAXWAVES];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int P = q.P, T = q.T, G = q.G, K = q.K, R = K / 2;
  float* Wn = ws + ((size_t)b * q.LAT + c) * ws_bwd_floats(P, T, q.steps);
  float* inv = Wn + (size_t)T * P;
  float* st = inv + P;                       // x_s,     s = 0 .. steps-1
  float* gs = st + (size_t)q.steps * P;      // g_{s+1}, s = 0 .. steps-1
  forward_body(q, lds, x_hp, depth, reg_w, reg_b, enc_w, enc_b, Wn, inv, st, b, c);
  // forward_body ended on a barrier: the LDS state is dead, the two buffers now carry the gradient
  for (int p = tid; p < P; p += blockDim.x) lds[p] = g4[((size_t)b * q.LAT + c) * P + p];
  __syncthreads();
  int cur = 0;
  for (int step = q.steps - 1; step >= 0; --step) {
    const float* g = lds + cur * P;
    float* gn = lds + (cur ^ 1) * P;
    for (int p = tid; p < P; p += blockDim.x) {
      const int py = p / G, px = p % G;
      gs[(size_t)step * P + p] = g[p];
      // g_s[p] = sum_t Wn[t][p - off(t)] * g_{s+1}[p - off(t)]   (gather form)
      float acc = 0.f;
      for (int ky = 0; ky < K; ++ky) {
        const int sy = py - (ky - R);
        if (sy < 0 || sy >= G) continue;
        for (int kx = 0; kx < K; ++kx) {
          const int sx = px - (kx - R);
          if (sx < 0 || sx >= G) continue;
          acc += Wn[(size_t)(ky * K + kx) * P + sy * G + sx] * g[sy * G + sx];
        }
      }
      gn[p] = acc;
    }
    __syncthreads();
    cur ^= 1;
  }
  // initial state x0 = enc_w[c] * d + enc_b[c]
  {
    const float* g0 = lds + cur * P;
    float a = 0.f, bs = 0.f;
    for (int p = tid; p < P; p += blockDim.x) { a += g0[p] * depth_sample(q, depth, b, p); bs += g0[p]; }
    a = block_sum(a, red);
    bs = block_sum(bs, red);
    if (tid == 0) { atomicAdd(&d_enc_w[c], a); atomicAdd(&d_enc_b[c], bs); }
  }
  if (q.steps == 0) return;                  // no propagation: the regressor is not on the path, its gradients stay exact zeros
  // dWn[t][p] = sum_s g_{s+1}[p] * x_s[p + off(t)], then through Wn = W * inv and the sigmoid: dz = (dWn - <dWn, Wn>) inv W (1 - W).
  // Thread p is the only reader and writer of column p of Wn from here on.
  for (int p = tid; p < P; p += blockDim.x) {
    const int py = p / G, px = p % G;
    float x[3];
    hp_sample(q, x_hp, b, p, x);
    lds[p] = x[0]; lds[MAXP + p] = x[1]; lds[2 * MAXP + p] = x[2];   // g0 was consumed before block_sum's barriers
    float dot = 0.f;
    for (int ky = 0; ky < K; ++ky) {
      for (int kx = 0; kx < K; ++kx) {
        const int t = ky * K + kx, yy = py + ky - R, xq = px + kx - R;
        float a = 0.f;
        if (yy >= 0 && yy < G && xq >= 0 && xq < G)
          for (int s = 0; s < q.steps; ++s) a += gs[(size_t)s * P + p] * st[(size_t)s * P + yy * G + xq];
        dot += a * Wn[(size_t)t * P + p];
        Wn[(size_t)t * P + p] = a;
      }
    }
    const float iv = inv[p];
    for (int t = 0; t < T; ++t) {
      const float* w = reg_w + (size_t)(c * T + t) * 3;
      const float v = sigmoidf(w[0] * x[0] + w[1] * x[1] + w[2] * x[2] + reg_b[c * T + t]);
      Wn[(size_t)t * P + p] = (Wn[(size_t)t * P + p] - dot) * iv * v * (1.f - v);   // dz
    }
  }
  __syncthreads();
  const int nw = blockDim.x >> 6, lane = tid & 63;
  for (int t = tid >> 6; t < T; t += nw) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, ab = 0.f;
    for (int p = lane; p < P; p += 64) {
      const float dz = Wn[(size_t)t * P + p];
      a0 += dz * lds[p]; a1 += dz * lds[MAXP + p]; a2 += dz * lds[2 * MAXP + p]; ab += dz;
    }
    a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); ab = wave_sum(ab);
    if (lane == 0) {
      float* dw = d_reg_w + (size_t)(c * T + t) * 3;
      atomicAdd(&dw[0], a0); atomicAdd(&dw[1], a1); atomicAdd(&dw[2], a2);
      atomicAdd(&d_reg_b[c * T + t], ab);
    }
  }
}

// ---- tail: e2 = conv1x1_{LAT->3}(x4) on the GxG grid, out = bilinear_{G->S}(e2) + image.  A workgroup owns `rows` output rows of one
// (image, output channel) plane and mixes only the grid rows those touch.
__global__ __launch_bounds__(256) void diffuse_tail_cfg_fwd_kernel(const float* __restrict__ x4, const float* __restrict__ cw,
                                                                   const float* __restrict__ cb, const float* __restrict__ image,
                                                                   float* __restrict__ out, int S, int G, int LAT, int rows) {
  __shared__ float e2[MAXP];
  const int bo = blockIdx.y, b = bo / 3, o = bo % 3, tid = threadIdx.x, P = G * G;
  const int r0 = blockIdx.x * rows, r1 = min(S, r0 + rows);
  if (r0 >= r1) return;
  const float scale = (float)G / (float)S;
  int ylo, yhi, tmp; float ltmp;
  bilinear_src(r0, scale, G, ylo, tmp, ltmp);
  bilinear_src(r1 - 1, scale, G, tmp, yhi, ltmp);
  const int ncell = (yhi - ylo + 1) * G;      // <= P
  for (int i = tid; i < ncell; i += blockDim.x) {
    const int cell = ylo * G + i;
    float acc = cb[o];
    for (int c = 0; c < LAT; ++c) acc += cw[o * LAT + c] * x4[((size_t)b * LAT + c) * P + cell];
    e2[i] = acc;
  }
  __syncthreads();
  const size_t plane = (size_t)bo * S * S;
  const int q4 = S / 4;  // float4 per row
  for (int i = tid; i < (r1 - r0) * q4; i += blockDim.x) {
    const int y = r0 + i / q4, xq = (i % q4) * 4;
    int y0, y1; float ly;
    bilinear_src(y, scale, G, y0, y1, ly);
    y0 -= ylo; y1 -= ylo;
    f32x4 im = *reinterpret_cast<const f32x4*>(image + plane + (size_t)y * S + xq);
    f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int x0, x1; float lx;
      bilinear_src(xq + j, scale, G, x0, x1, lx);
      const float v = (1.f - ly) * ((1.f - lx) * e2[y0 * G + x0] + lx * e2[y0 * G + x1]) +
                      ly * ((1.f - lx) * e2[y1 * G + x0] + lx * e2[y1 * G + x1]);
      r[j] = v + im[j];
    }
    *reinterpret_cast<f32x4*>(out + plane + (size_t)y * S + xq) = r;
  }
}

// ge2[b][o][cell] = sum over pixels of bilinear weight(pixel -> cell) * gout   (gather per cell, fixed order)
__global__ __launch_bounds__(256) void diffuse_tail_cfg_bwd_cells_kernel(const float* __restrict__ gout, float* __restrict__ ge2,
                                                                         int S, int G) {
  __shared__ float red[MAXWAVES];
  const int cell = blockIdx.x, bo = blockIdx.y, cy = cell / G, cx = cell % G, tid = threadIdx.x;
  const float scale = (float)G / (float)S;
  // pixel range that can touch this cell: src in (c-1, c+1)  ->  dst in ((c-0.5)/scale - 0.5, (c+1.5)/scale - 0.5); clamp handles borders
  const int lo_y = max(0, (int)floorf((cy - 0.5f) / scale - 0.5f) - 1), hi_y = min(S - 1, (int)ceilf((cy + 1.5f) / scale - 0.5f) + 1);
  const int lo_x = max(0, (int)floorf((cx - 0.5f) / scale - 0.5f) - 1), hi_x = min(S - 1, (int)ceilf((cx + 1.5f) / scale - 0.5f) + 1);
  const int ny = hi_y - lo_y + 1, nx = hi_x - lo_x + 1;
  const float* gp = gout + (size_t)bo * S * S;
  float acc = 0.f;
  for (int i = tid; i < ny * nx; i += blockDim.x) {
    const int y = lo_y + i / nx, x = lo_x + i % nx;
    int y0, y1, x0, x1; float ly, lx;
    bilinear_src(y, scale, G, y0, y1, ly);
    bilinear_src(x, scale, G, x0, x1, lx);
    const float wy = (y0 == cy ? 1.f - ly : 0.f) + (y1 == cy ? ly : 0.f);
    const float wx = (x0 == cx ? 1.f - lx : 0.f) + (x1 == cx ? lx : 0.f);
    const float w = wy * wx;
    if (w != 0.f) acc += w * gp[(size_t)y * S + x];
  }
  acc = block_sum(acc, red);
  if (tid == 0) ge2[(size_t)bo * G * G + cell] = acc;
}

// g4 = cw^T ge2 ; d_cw += ge2 x4^T ; d_cb += sum ge2     (one workgroup per (image, latent channel))
__global__ __launch_bounds__(256) void diffuse_tail_cfg_bwd_mix_kernel(const float* __restrict__ ge2, const float* __restrict__ x4,
                                                                       const float* __restrict__ cw, float* __restrict__ g4,
                                                                       float* __restrict__ d_cw, float* __restrict__ d_cb, int P, int LAT) {
  __shared__ float red[MAXWAVES];
  const int c = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* ge = ge2 + (size_t)b * 3 * P;
  const size_t row = ((size_t)b * LAT + c) * P;
  const float w0 = cw[c], w1 = cw[LAT + c], w2 = cw[2 * LAT + c];
  float a[3] = {0.f, 0.f, 0.f}, s[3] = {0.f, 0.f, 0.f};
  for (int p = tid; p < P; p += blockDim.x) {
    const float e0 = ge[p], e1 = ge[P + p], e2 = ge[2 * (size_t)P + p], x = x4[row + p];
    g4[row + p] = w0 * e0 + w1 * e1 + w2 * e2;
    a[0] += e0 * x; a[1] += e1 * x; a[2] += e2 * x;
    s[0] += e0; s[1] += e1; s[2] += e2;
  }
#pragma unroll
  for (int o = 0; o < 3; ++o) {
    const float v = block_sum(a[o], red);
    if (tid == 0) atomicAdd(&d_cw[o * LAT + c], v);
  }
  if (c == 0) {
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      const float v = block_sum(s[o], red);
      if (tid == 0) atomicAdd(&d_cb[o], v);
    }
  }
}

bool tail_in_domain(int B, int S, int G, int LAT) {
  return B > 0 && S >= 4 && S % 4 == 0 && G >= 2 && G <= MAXG && LAT >= 1 && LAT <= MAXLAT;
}
bool in_domain(int B, int S, int G, int K, int steps, int LAT) {
  return tail_in_domain(B, S, G, LAT) && K >= 3 && K <= MAXK && (K & 1) && steps >= 0 && steps <= MAXSTEPS;
}
#define CFG_REQUIRE(name) DGTD_REQUIRE(in_domain(B, S, G, K, steps, LAT), name ": outside the domain (B > 0, S a positive multiple of 4, " \
    "2 <= G <= 64, odd 3 <= K <= 11, 0 <= steps <= 64, 1 <= LAT <= 64): B=%d S=%d G=%d K=%d steps=%d LAT=%d", B, S, G, K, steps, LAT)
#define TAIL_REQUIRE(name) DGTD_REQUIRE(tail_in_domain(B, S, G, LAT), name ": outside the domain (B > 0, S a positive multiple of 4, " \
    "2 <= G <= 64, 1 <= LAT <= 64): B=%d S=%d G=%d LAT=%d", B, S, G, LAT)

// threads per workgroup of the state kernels: one per cell, whole waves, at most 1024 (larger grids loop)
int state_threads(int P) { return (int)std::min<int64_t>(1024, cdiv(P, 64) * 64); }

}  // namespace

extern "C" int64_t dgtd_diffuser_cfg_workspace(int B, int S, int G, int K, int steps, int LAT, int backward) {
  if (!in_domain(B, S, G, K, steps, LAT)) return -1;
  const int P = G * G, T = K * K;
  const size_t per = backward ? ws_bwd_floats(P, T, steps) : ws_fwd_floats(P, T);
  return (int64_t)((size_t)B * LAT * per * sizeof(float));
}

extern "C" int dgtd_diffuser_cfg_fwd(const float* x_hp, const float* depth, const float* reg_w, const float* reg_b,
                                     const float* enc_w, const float* enc_b, float* x4, void* workspace, int B, int S, int G, int K,
                                     int steps, int LAT, dgtd_stream s) {
  // inputs + output, and the normalised weights written once and read once per step
  DGTD_PROF(s, DGTD_HBM, 4.0 * B * (4.0 * G * G + (double)LAT * G * G * (1.0 + (steps > 0 ? (1.0 + steps) * K * K : 0.0))),
            "dgtd_diffuser_cfg_fwd[B=%d,S=%d,G=%d,K=%d,steps=%d,LAT=%d]", B, S, G, K, steps, LAT);
  CFG_REQUIRE("diffuser_cfg_fwd");
  DGTD_REQUIRE(workspace != nullptr || steps == 0, "diffuser_cfg_fwd: workspace is null");
  const Cfg q{S, G, G * G, K, K * K, steps, LAT};
  hipLaunchKernelGGL(diffuser_cfg_fwd_kernel, dim3(LAT, B), dim3(state_threads(q.P)), 0, (hipStream_t)s, x_hp, depth, reg_w, reg_b,
                     enc_w, enc_b, x4, (float*)workspace, q);
  DGTD_CHECK_LAUNCH("diffuser_cfg_fwd");
  return 0;
}

extern "C" int dgtd_diffuser_cfg_bwd(const float* x_hp, const float* depth, const float* reg_w, const float* reg_b,
                                     const float* enc_w, const float* enc_b, const float* g4, float* d_reg_w, float* d_reg_b,
                                     float* d_enc_w, float* d_enc_b, void* workspace, int B, int S, int G, int K, int steps, int LAT,
                                     dgtd_stream s) {
  // the weights written once, read once per forward and per backward step, dz written and read; states and gradients written and read
  DGTD_PROF(s, DGTD_HBM, 4.0 * B * (4.0 * G * G + (double)LAT * G * G * (1.0 + (steps > 0 ? (3.0 + 2.0 * steps) * K * K + 4.0 * steps : 0.0))),
            "dgtd_diffuser_cfg_bwd[B=%d,S=%d,G=%d,K=%d,steps=%d,LAT=%d]", B, S, G, K, steps, LAT);
  CFG_REQUIRE("diffuser_cfg_bwd");
  DGTD_REQUIRE(workspace != nullptr || steps == 0, "diffuser_cfg_bwd: workspace is null");
  const Cfg q{S, G, G * G, K, K * K, steps, LAT};
  hipLaunchKernelGGL(diffuser_cfg_bwd_kernel, dim3(LAT, B), dim3(state_threads(q.P)), 0, (hipStream_t)s, x_hp, depth, reg_w, reg_b,
                     enc_w, enc_b, g4, d_reg_w, d_reg_b, d_enc_w, d_enc_b, (float*)workspace, q);
  DGTD_CHECK_LAUNCH("diffuser_cfg_bwd");
  return 0;
}

extern "C" int dgtd_diffuse_tail_cfg_fwd(const float* x4, const float* cw, const float* cb, const float* image, float* out,
                                         int B, int S, int G, int LAT, dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, 2.0 * 4 * B * 3 * S * S + 4.0 * B * LAT * G * G, "dgtd_diffuse_tail_cfg_fwd[B=%d,S=%d,G=%d,LAT=%d]", B, S, G, LAT);
  TAIL_REQUIRE("diffuse_tail_cfg_fwd");
  const int rows = (int)std::min<int64_t>(S, cdiv(1024, S / 4));   // about four float4 per thread
  hipLaunchKernelGGL(diffuse_tail_cfg_fwd_kernel, dim3((unsigned)cdiv(S, rows), 3 * B), dim3(256), 0, (hipStream_t)s, x4, cw, cb, image,
                     out, S, G, LAT, rows);
  DGTD_CHECK_LAUNCH("diffuse_tail_cfg_fwd");
  return 0;
}

extern "C" int64_t dgtd_diffuse_tail_cfg_bwd_workspace(int B, int G) { return (int64_t)B * 3 * G * G * sizeof(float); }

extern "C" int dgtd_diffuse_tail_cfg_bwd(const float* gout, const float* x4, const float* cw, float* g4, float* d_cw, float* d_cb,
                                         void* workspace, int B, int S, int G, int LAT, dgtd_stream s) {
  DGTD_PROF(s, DGTD_HBM, 4.0 * B * 3 * S * S + 2.0 * 4 * B * LAT * G * G, "dgtd_diffuse_tail_cfg_bwd[B=%d,S=%d,G=%d,LAT=%d]", B, S, G, LAT);
  TAIL_REQUIRE("diffuse_tail_cfg_bwd");
  DGTD_REQUIRE(workspace != nullptr, "diffuse_tail_cfg_bwd: workspace is null");
  float* ge2 = (float*)workspace;
  // a cell gathers about (2 S / G + 3)^2 pixels: one wave when that is small, four otherwise
  const int span = 2 * S / G + 3, threads = span * span > 1024 ? 256 : 64;
  hipLaunchKernelGGL(diffuse_tail_cfg_bwd_cells_kernel, dim3(G * G, 3 * B), dim3(threads), 0, (hipStream_t)s, gout, ge2, S, G);
  DGTD_CHECK_LAUNCH("diffuse_tail_cfg_bwd_cells");
  hipLaunchKernelGGL(diffuse_tail_cfg_bwd_mix_kernel, dim3(LAT, B), dim3(256), 0, (hipStream_t)s, (const float*)ge2, x4, cw, g4, d_cw,
                     d_cb, G * G, LAT);
  DGTD_CHECK_LAUNCH("diffuse_tail_cfg_bwd_mix");
  return 0;
}
