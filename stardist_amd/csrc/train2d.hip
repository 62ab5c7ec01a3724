// train2d.hip -- the backward pass and the losses of StarDist2D training (stardist/models/model2d.py train, base.py:34-60, 315-325).
//
//   * k_wgrad: weight gradient of a 'same' 3x3 or 1x1 convolution, channels-last f32, batch B, as a GEMM with K = pixels on the
//     f32 matrix cores (v_mfma_f32_32x32x2_f32, exact f32):
//         dW[co][ci][ky][kx] = sum_{b,y,x} g[b][y][x][co] * in[b][y+ky-1][x+kx-1][ci]        (zero outside the image)
//     The input takes the forward kernels' two-source form [up-sampled src0 | src1], so the first convolution of an up level gets its
//     gradient without the concatenation being written.  A workgroup owns (pixel chunk, 32 output channels, 32 input channels): per
//     8 x 32 tile it stages the gradient tile and the input tile (3x3: plus its halo) in LDS once and runs all taps on them.  The pixels are
//     split into a number of chunks that depends on the shape only; each chunk writes its partial sums to the workspace and
//     k_wgrad_reduce adds them in chunk order (float64).  No atomics: two calls give the same bits.
//   * k_relu_mask: the adjoint of ReLU.  Those of MaxPooling2D and UpSampling2D + Concatenate (sd_maxpool_adjoint_ndhwc_device,
//     sd_upcat_adjoint_ndhwc_device) are the depth-1 case of the 3D kernels and live next to them in train3d.hip.
//   * sd_stardist_loss2d_device: the two losses of the 2D model and their gradients in three passes -- per-block float64 partial sums
//     over fixed pixel ranges, one block that adds them in order, then the per-pixel gradients.
//   * sd_stardist_loss2d_metrics_device: the same passes, the first two also summing the reference's Keras metrics (kld, relevant_mae,
//     relevant_mse, dist_iou_metric) over the loads the losses make; the losses and gradients are those of the entry above, bit for bit.
#include "common.h"
#include "stardist_hip.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WG_TH = 8, WG_TW = 32, WG_PIX = WG_TH * WG_TW;   // output tile: 8 rows x 32 columns of one sample
constexpr int WG_PS = 33;                                        // floats per pixel in LDS (32 channels + 1: distinct banks for the two lane halves)
constexpr int WG_THREADS = 256;

struct WgradParams {
  const float* g;          // [B][H][W][c_out]
  const float* s0;         // [B][H >> sy0][W >> sx0][c0]
  const float* s1;         // [B][H >> sy1][W >> sx1][c1] (c1 == 0: unused)
  float* ws;               // [n_chunks][taps][co_pad][ci_pad]
  float* wsb;              // [n_chunks][co_pad] (bias partials)
  int c_out, c0, c1, sy0, sx0, sy1, sx1;
  int B, H, W, k;          // k = 3 or 1
  int tiles_y, tiles_x, n_tiles, tiles_per_chunk, co_pad, ci_pad;
};

__device__ __forceinline__ float load_in(const WgradParams& P, int b, int Y, int X, int ci) {
  if (Y < 0 || Y >= P.H || X < 0 || X >= P.W) return 0.f;
  if (ci < P.c0) {
    const int H0 = P.H >> P.sy0, W0 = P.W >> P.sx0;
    return P.s0[(((long long)b * H0 + (Y >> P.sy0)) * W0 + (X >> P.sx0)) * P.c0 + ci];
  }
  ci -= P.c0;
  if (ci >= P.c1) return 0.f;
  const int H1 = P.H >> P.sy1, W1 = P.W >> P.sx1;
  return P.s1[(((long long)b * H1 + (Y >> P.sy1)) * W1 + (X >> P.sx1)) * P.c1 + ci];
}

template <int K>
__global__ __launch_bounds__(WG_THREADS) void k_wgrad(WgradParams P) {
  constexpr int TAPS = K * K;
  constexpr int PAD = K / 2;                                     // halo: 1 for the 3x3 layers, none for the 1x1 heads
  constexpr int HH = WG_TH + 2 * PAD, HW = WG_TW + 2 * PAD;
  __shared__ float gL[WG_PIX * WG_PS];
  __shared__ float inL[HH * HW * WG_PS];
  const int chunk = blockIdx.x, cg = blockIdx.y, cc = blockIdx.z;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l32 = lane & 31, h = lane >> 5;
  const int c_in = P.c0 + P.c1;
  f32x16 acc[TAPS];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
  float bsum = 0.f;
  const int t_begin = chunk * P.tiles_per_chunk;
  const int t_end = min(P.n_tiles, t_begin + P.tiles_per_chunk);
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int b = tile / (P.tiles_y * P.tiles_x);
    const int rem = tile - b * P.tiles_y * P.tiles_x;
    const int y0 = (rem / P.tiles_x) * WG_TH, x0 = (rem % P.tiles_x) * WG_TW;
    __syncthreads();                               // the previous tile's operands are consumed
    for (int e = tid; e < WG_PIX * 32; e += WG_THREADS) {
      const int p = e >> 5, c = e & 31, co = cg * 32 + c;
      const int y = y0 + p / WG_TW, x = x0 + p % WG_TW;
      float v = 0.f;
      if (y < P.H && x < P.W && co < P.c_out) v = P.g[(((long long)b * P.H + y) * P.W + x) * P.c_out + co];
      gL[p * WG_PS + c] = v;
    }
    for (int e = tid; e < HH * HW * 32; e += WG_THREADS) {
      const int hp = e >> 5, c = e & 31, ci = cc * 32 + c;
      const int Y = y0 - PAD + hp / HW, X = x0 - PAD + hp % HW;
      inL[hp * WG_PS + c] = ci < c_in ? load_in(P, b, Y, X, ci) : 0.f;
    }
    __syncthreads();
    if (cc == 0 && tid < 32) {                     // bias partial: the tile's pixels in order
      for (int p = 0; p < WG_PIX; ++p) bsum += gL[p * WG_PS + tid];
    }
    // wave w: tile rows 2w, 2w + 1; k step s takes pixels 2s (lane half 0) and 2s + 1 (lane half 1) of those 64
#pragma unroll 2
    for (int s = 0; s < 32; ++s) {
      const int pp = 2 * s + h;
      const int r = 2 * wave + (pp >> 5), x = pp & 31;
      const float a = gL[(r * WG_TW + x) * WG_PS + l32];
#pragma unroll
      for (int t = 0; t < TAPS; ++t) {
        const int dy = t / K, dx = t % K;
        const float bv = inL[((r + dy) * HW + x + dx) * WG_PS + l32];
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc[t], 0, 0, 0);
      }
    }
  }
  // the four waves' sums, added in wave order, tap by tap
  const size_t cstride = (size_t)P.co_pad * P.ci_pad;
  float* red = gL;                                  // 3 x 1024 floats
#pragma unroll
  for (int t = 0; t < TAPS; ++t) {
    __syncthreads();
    if (wave > 0)
#pragma unroll
      for (int q = 0; q < 16; ++q) red[(wave - 1) * 1024 + q * 64 + lane] = acc[t][q];
    __syncthreads();
    if (wave == 0) {
      float* dst = P.ws + ((size_t)chunk * TAPS + t) * cstride;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float v = ((acc[t][q] + red[q * 64 + lane]) + red[1024 + q * 64 + lane]) + red[2048 + q * 64 + lane];
        const int co = cg * 32 + (q & 3) + 8 * (q >> 2) + 4 * h, ci = cc * 32 + l32;
        dst[(size_t)co * P.ci_pad + ci] = v;
      }
    }
  }
  if (cc == 0 && tid < 32) P.wsb[(size_t)chunk * P.co_pad + cg * 32 + tid] = bsum;
}

// dW[co][ci][tap] = sum over chunks (ascending) of the partials; db[co] likewise
__global__ void k_wgrad_reduce(const float* __restrict__ ws, const float* __restrict__ wsb, int n_chunks, int taps, int c_out, int c_in,
                               int co_pad, int ci_pad, float* __restrict__ dw, float* __restrict__ db) {
  const long long n = (long long)taps * c_out * c_in;
  const size_t cstride = (size_t)taps * co_pad * ci_pad;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < n + c_out; idx += (long long)gridDim.x * blockDim.x) {
    if (idx < n) {
      const int ci = (int)(idx % c_in);
      const long long r = idx / c_in;
      const int co = (int)(r % c_out), t = (int)(r / c_out);
      const size_t off = ((size_t)t * co_pad + co) * ci_pad + ci;
      double s = 0.0;
      for (int c = 0; c < n_chunks; ++c) s += (double)ws[c * cstride + off];
      dw[((size_t)co * c_in + ci) * taps + t] = (float)s;
    } else if (db) {
      const int co = (int)(idx - n);
      double s = 0.0;
      for (int c = 0; c < n_chunks; ++c) s += (double)wsb[(size_t)c * co_pad + co];
      db[co] = (float)s;
    }
  }
}

__global__ void k_relu_mask(const float* __restrict__ dy, const float* __restrict__ y, long long n, float* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    out[i] = y[i] > 0.f ? dy[i] : 0.f;
}

// ---- losses -------------------------------------------------------------------------------------------------------------------
constexpr int LOSS_THREADS = 256;
constexpr int LOSS_PIX_PER_BLOCK = 4096;
constexpr int LOSS_TERMS = 5;        // unmasked pixels, sum BCE, sum dist mask, sum mean_rays(mask * pen), sum mean_rays((1 - mask) |d|)
constexpr int METRIC_TERMS = 4;      // the metrics pass adds: sum kld, sum m mean_r |e|, sum m mean_r e^2, sum m iou
constexpr double K_EPS = 1e-7;       // Keras' epsilon()

__device__ __forceinline__ double bce_clipped(double t, double p) {
  const double pc = fmin(fmax(p, K_EPS), 1.0 - K_EPS);
  return -(t * log(pc + K_EPS) + (1.0 - t) * log(1.0 - pc + K_EPS));
}

// METRICS adds the sums of the Keras metrics the reference compiles its model with (base.py:68-104, 351-353) over the same loads:
//     [5] kld: bce(tc, pc) - bce(tc, tc) over the pixels with prob_true >= 0   (tc = clip(prob_true, e, 1), pc = clip(prob, e, 1))
//     [6] m mean_r |t_r - d_r|   [7] m mean_r (t_r - d_r)^2   [8] m inter / (union + e),  inter / union = mean_r min / max(t_r, d+_r)^2
// (d+ = max(0, d)); METRICS = false is the losses' pass alone.
template <bool METRICS>
__global__ __launch_bounds__(LOSS_THREADS) void k_loss_partials(const float* __restrict__ prob, const float* __restrict__ dist,
                                                                const float* __restrict__ pt, const float* __restrict__ dtm, long long n_pix,
                                                                int R, int mse, double* __restrict__ part) {
  constexpr int T = METRICS ? LOSS_TERMS + METRIC_TERMS : LOSS_TERMS;
  __shared__ double sh[T][LOSS_THREADS];
  double acc[T] = {};
  const long long p0 = (long long)blockIdx.x * LOSS_PIX_PER_BLOCK;
  const long long p1 = min(n_pix, p0 + LOSS_PIX_PER_BLOCK);
  for (long long p = p0 + threadIdx.x; p < p1; p += LOSS_THREADS) {
    const double t = pt[p];
    if (t >= 0) {
      acc[0] += 1.0; acc[1] += bce_clipped(t, (double)prob[p]);
      if constexpr (METRICS) {
        const double tc = fmin(fmax(t, K_EPS), 1.0), pc = fmin(fmax((double)prob[p], K_EPS), 1.0);
        acc[5] += bce_clipped(tc, pc) - bce_clipped(tc, tc);
      }
    }
    const float* tr = dtm + p * (R + 1);
    const float* d = dist + p * R;
    const double m = tr[R];
    acc[2] += m;
    double sa = 0, sr = 0;
    double ma = 0, ms = 0, in = 0, un = 0;
    for (int r = 0; r < R; ++r) {
      const double e = (double)((float)tr[r] - d[r]);
      sa += m * (mse ? e * e : fabs(e));
      sr += (1.0 - m) * fabs((double)d[r]);
      if constexpr (METRICS) {
        const double tt = tr[r], dp = fmax(0.0, (double)d[r]);
        const double lo = fmin(tt, dp), hi = fmax(tt, dp);
        ma += fabs(e);
        ms += e * e;
        in += lo * lo;
        un += hi * hi;
      }
    }
    acc[3] += sa / R;
    acc[4] += sr / R;
    if constexpr (METRICS) {
      acc[6] += m * (ma / R);
      acc[7] += m * (ms / R);
      acc[8] += m * ((in / R) / (un / R + K_EPS));
    }
  }
#pragma unroll
  for (int k = 0; k < T; ++k) sh[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int s = LOSS_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
#pragma unroll
      for (int k = 0; k < T; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x < T) part[(size_t)blockIdx.x * T + threadIdx.x] = sh[threadIdx.x][0];
}

// one thread: the block partials in block order -> losses {prob, dist, total} and the two scale factors of the gradients; METRICS: also
// the metrics {kld, relevant_mae, relevant_mse, dist_iou_metric} of the batch (Keras' per-pixel means over n_pix, the kld over the
// unmasked pixels)
template <bool METRICS>
__global__ void k_loss_finish(const double* __restrict__ part, int n_blocks, long long n_pix, double w_prob, double w_dist, double reg,
                              double* __restrict__ losses, double* __restrict__ scal, double* __restrict__ metrics) {
  constexpr int T = METRICS ? LOSS_TERMS + METRIC_TERMS : LOSS_TERMS;
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s[T] = {};
  for (int b = 0; b < n_blocks; ++b)
    for (int k = 0; k < T; ++k) s[k] += part[(size_t)b * T + k];
  const double prob_loss = s[1] / s[0];
  const double norm = s[2] / (double)n_pix + K_EPS;                // K.mean(mask) + K.epsilon()
  const double dist_loss = (s[3] / norm + (reg > 0 ? reg * s[4] : 0.0)) / (double)n_pix;
  losses[0] = prob_loss;
  losses[1] = dist_loss;
  losses[2] = w_prob * prob_loss + w_dist * dist_loss;
  scal[0] = w_prob / s[0];
  scal[1] = w_dist / ((double)n_pix * norm);
  scal[2] = reg > 0 ? w_dist * reg / (double)n_pix : 0.0;
  if constexpr (METRICS) {
    metrics[0] = s[5] / s[0];
    for (int k = 1; k < METRIC_TERMS; ++k) metrics[k] = (s[5 + k] / (double)n_pix) / norm;
  }
}

__global__ void k_loss_grad(const float* __restrict__ prob, const float* __restrict__ dist, const float* __restrict__ pt,
                            const float* __restrict__ dtm, long long n_pix, int R, int mse, const double* __restrict__ scal,
                            float* __restrict__ gz, float* __restrict__ gd) {
  const double sp = scal[0], sd = scal[1] / R, sr = scal[2] / R;
  const long long n = n_pix * R;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n + n_pix; i += (long long)gridDim.x * blockDim.x) {
    if (i < n) {
      const long long p = i / R;
      const int r = (int)(i - p * R);
      const double m = dtm[p * (R + 1) + R];
      const float d = dist[i];
      const double e = (double)(d - dtm[p * (R + 1) + r]);          // d - t
      const double pen = mse ? 2.0 * e : (e > 0 ? 1.0 : (e < 0 ? -1.0 : 0.0));
      const double sg = d > 0 ? 1.0 : (d < 0 ? -1.0 : 0.0);
      gd[i] = (float)(sd * m * pen + sr * (1.0 - m) * sg);
    } else {
      const long long p = i - n;
      const double t = pt[p], q = prob[p];
      double g = 0.0;
      if (t >= 0 && q >= K_EPS && q <= 1.0 - K_EPS) {
        // d/dp of -(t log(p + eps) + (1 - t) log(1 - p + eps)), times the sigmoid's p (1 - p)
        const double dp = -t / (q + K_EPS) + (1.0 - t) / (1.0 - q + K_EPS);
        g = sp * dp * q * (1.0 - q);
      }
      gz[p] = (float)g;
    }
  }
}

inline unsigned grid_for(long long n, int threads = 256) {
  long long b = (n + threads - 1) / threads;
  return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

}  // namespace

extern "C" int sd_conv_wgrad_ndhwc_device(const float* d_g, int c_out, const float* d_src0, int c0, int up0, const float* d_src1, int c1, int up1,
                                          int B, int H, int W, int k, float* d_dw, float* d_db, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (!d_g || !d_src0 || !d_dw || c_out <= 0 || c0 <= 0 || c1 < 0 || (c1 > 0 && !d_src1) || B <= 0 || H <= 0 || W <= 0 || (k != 1 && k != 3) ||
      (up0 & ~3) || (up1 & ~3) || (((up0 | up1) & 1) && (W & 1)) || (((up0 | up1) & 2) && (H & 1)) || (k == 1 && (up0 || c1))) {
    sd::set_error("sd_conv_wgrad_ndhwc: kernel 3 or 1 (1: one full-resolution source), up bits 1 (x) / 2 (y) over even sizes, positive sizes");
    return -1;
  }
  WgradParams P;
  P.g = d_g; P.s0 = d_src0; P.s1 = d_src1; P.c_out = c_out; P.c0 = c0; P.c1 = c1;
  P.sx0 = up0 & 1; P.sy0 = (up0 >> 1) & 1; P.sx1 = up1 & 1; P.sy1 = (up1 >> 1) & 1;
  P.B = B; P.H = H; P.W = W; P.k = k;
  P.tiles_y = sd::div_up(H, WG_TH); P.tiles_x = sd::div_up(W, WG_TW);
  P.n_tiles = B * P.tiles_y * P.tiles_x;
  const int co_groups = sd::div_up(c_out, 32), ci_chunks = sd::div_up(c0 + c1, 32);
  P.co_pad = co_groups * 32; P.ci_pad = ci_chunks * 32;
  const int taps = k * k;
  // the pixel chunks: a function of the shape only (about 2048 workgroups, at most 2^24 partial floats)
  long long n_chunks = sd::div_up(2048, (long long)co_groups * ci_chunks);
  const long long per_chunk = (long long)taps * P.co_pad * P.ci_pad;
  const long long cap = (1LL << 24) / per_chunk;
  if (n_chunks > cap) n_chunks = cap;
  if (n_chunks < 1) n_chunks = 1;
  if (n_chunks > P.n_tiles) n_chunks = P.n_tiles;
  P.tiles_per_chunk = sd::div_up(P.n_tiles, n_chunks);
  n_chunks = sd::div_up(P.n_tiles, P.tiles_per_chunk);
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  P.ws = A.take_n<float>((size_t)n_chunks * per_chunk);
  P.wsb = A.take_n<float>((size_t)n_chunks * P.co_pad);
  if (!P.ws || !P.wsb) return -1;
  dim3 grid((unsigned)n_chunks, (unsigned)co_groups, (unsigned)ci_chunks);
  if (k == 3) hipLaunchKernelGGL(k_wgrad<3>, grid, dim3(WG_THREADS), 0, s, P);
  else hipLaunchKernelGGL(k_wgrad<1>, grid, dim3(WG_THREADS), 0, s, P);
  SD_LAUNCH_CHECK();
  const long long n = (long long)taps * c_out * (c0 + c1) + c_out;
  hipLaunchKernelGGL(k_wgrad_reduce, dim3(grid_for(n)), dim3(256), 0, s, P.ws, P.wsb, (int)n_chunks, taps, c_out, c0 + c1, P.co_pad, P.ci_pad,
                     d_dw, d_db);
  SD_LAUNCH_CHECK();
  return 0;
}

extern "C" int sd_relu_mask_device(const float* d_dy, const float* d_y, long long n, float* d_out, void* stream_) {
  if (n <= 0) return 0;
  if (!d_dy || !d_y || !d_out) { sd::set_error("sd_relu_mask: null pointer"); return -1; }
  hipLaunchKernelGGL(k_relu_mask, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream_, d_dy, d_y, n, d_out);
  SD_LAUNCH_CHECK();
  return 0;
}

namespace {

// the passes of both loss entry points (the arguments checked by the caller)
template <bool METRICS>
int loss2d_passes(const float* d_prob, const float* d_dist, const float* d_prob_true, const float* d_dist_true_mask, long long n_pix, int n_rays,
                  int dist_loss, double w_prob, double w_dist, double background_reg, double* d_losses, float* d_grad_logit, float* d_grad_dist,
                  double* d_metrics, hipStream_t s) {
  constexpr int T = METRICS ? LOSS_TERMS + METRIC_TERMS : LOSS_TERMS;
  const int n_blocks = sd::div_up(n_pix, LOSS_PIX_PER_BLOCK);
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  double* part = A.take_n<double>((size_t)n_blocks * T);
  double* scal = A.take_n<double>(4);
  if (!part || !scal) return -1;
  hipLaunchKernelGGL(k_loss_partials<METRICS>, dim3(n_blocks), dim3(LOSS_THREADS), 0, s, d_prob, d_dist, d_prob_true, d_dist_true_mask, n_pix,
                     n_rays, dist_loss, part);
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_loss_finish<METRICS>, dim3(1), dim3(64), 0, s, part, n_blocks, n_pix, w_prob, w_dist, background_reg, d_losses, scal,
                     d_metrics);
  SD_LAUNCH_CHECK();
  if (!d_grad_logit) return 0;                   // losses only
  hipLaunchKernelGGL(k_loss_grad, dim3(grid_for(n_pix * (n_rays + 1))), dim3(256), 0, s, d_prob, d_dist, d_prob_true, d_dist_true_mask, n_pix,
                     n_rays, dist_loss, scal, d_grad_logit, d_grad_dist);
  SD_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int sd_stardist_loss2d_device(const float* d_prob, const float* d_dist, const float* d_prob_true, const float* d_dist_true_mask,
                                         long long n_pix, int n_rays, int dist_loss, double w_prob, double w_dist, double background_reg,
                                         double* d_losses, float* d_grad_logit, float* d_grad_dist, void* stream_) {
  if (!d_prob || !d_dist || !d_prob_true || !d_dist_true_mask || !d_losses || n_pix <= 0 || n_rays <= 0 ||
      (dist_loss != 0 && dist_loss != 1) || (!d_grad_logit) != (!d_grad_dist)) {
    sd::set_error("sd_stardist_loss2d: dist_loss 0 (mae) or 1 (mse), positive sizes, inputs and d_losses given, both gradient buffers or neither");
    return -1;
  }
  return loss2d_passes<false>(d_prob, d_dist, d_prob_true, d_dist_true_mask, n_pix, n_rays, dist_loss, w_prob, w_dist, background_reg, d_losses,
                              d_grad_logit, d_grad_dist, nullptr, (hipStream_t)stream_);
}

extern "C" int sd_stardist_loss2d_metrics_device(const float* d_prob, const float* d_dist, const float* d_prob_true,
                                                 const float* d_dist_true_mask, long long n_pix, int n_rays, int dist_loss, double w_prob,
                                                 double w_dist, double background_reg, double* d_losses, float* d_grad_logit, float* d_grad_dist,
                                                 double* d_metrics, void* stream_) {
  if (!d_prob || !d_dist || !d_prob_true || !d_dist_true_mask || !d_losses || !d_metrics || n_pix <= 0 || n_rays <= 0 ||
      (dist_loss != 0 && dist_loss != 1) || (!d_grad_logit) != (!d_grad_dist)) {
    sd::set_error("sd_stardist_loss2d_metrics: dist_loss 0 (mae) or 1 (mse), positive sizes, inputs, d_losses and d_metrics given, both "
                  "gradient buffers or neither");
    return -1;
  }
  return loss2d_passes<true>(d_prob, d_dist, d_prob_true, d_dist_true_mask, n_pix, n_rays, dist_loss, w_prob, w_dist, background_reg, d_losses,
                             d_grad_logit, d_grad_dist, d_metrics, (hipStream_t)stream_);
}
