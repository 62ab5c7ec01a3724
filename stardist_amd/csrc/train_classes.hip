// train_classes.hip -- what training a multi-class model adds to a step (the reference's StarDistData2D / StarDistData3D with
// n_classes, stardist/models/model2d.py:106-119, and weighted_categorical_crossentropy, stardist/models/base.py:108-126).
//
//   * sd_class_targets_device: prob_class of a batch in one launch from the label patches uploaded for the other targets:
//     mask_to_categorical (stardist/utils.py:318-380) per pixel through a per-sample table label id -> class code, the nearest-neighbour
//     zoom by 1 / grid as one gather table per axis (built on the host from scipy.ndimage.zoom itself, -1 = scipy reads outside the
//     array and fills 0), the negative-label mask.  The same launch looks every label of the patches up once: one that the sample's
//     dict does not hold raises *d_missing with an atomic, which the caller reads where it synchronises anyway.
//   * sd_class_loss_device: the weighted categorical cross entropy on the logits of the class head and its gradient; the softmax is
//     never written.  float64 per pixel, per-block partial sums over fixed pixel ranges, one thread adds them in block order: no atomics,
//     the same bits on every call, with or without the gradient.
#include "common.h"
#include "stardist_hip.h"

namespace {

// ---- targets ------------------------------------------------------------------------------------------------------------------
constexpr int CODE_IGNORE = -1;      // class id None: every channel -1 (the background channel excepted)
constexpr int CODE_MISSING = -2;     // the label is not in the sample's dict

struct ClassTargetParams {
  const int* lab;            // [B][D][H][W], negative ids clipped to 0
  const int* meta;           // [B][4]: offset into keys / codes, entries, 1 = sorted keys (0 = dense: the id is the index), default code
  const int* keys;           // sorted label ids of the sparse tables (may be NULL when every table is dense)
  const int* codes;          // class codes: 0 ... n_classes, CODE_IGNORE, CODE_MISSING
  const int* tz;             // [d], [h], [w]: the source index along each axis, -1 = outside
  const int* ty;
  const int* tx;
  const unsigned char* neg;  // [B][d][h][w] or NULL
  float* out;                // [B][d][h][w][C]
  int* missing;
  int B, D, H, W, d, h, w, C;
};

__device__ __forceinline__ int class_code(const ClassTargetParams& P, int b, int label) {
  const int off = P.meta[4 * b], n = P.meta[4 * b + 1], sparse = P.meta[4 * b + 2], dflt = P.meta[4 * b + 3];
  if (!sparse) return label < n ? P.codes[off + label] : dflt;
  int lo = 0, hi = n;                                   // the first key >= label
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (P.keys[off + mid] < label) lo = mid + 1; else hi = mid;
  }
  return (lo < n && P.keys[off + lo] == label) ? P.codes[off + lo] : dflt;
}

__global__ void k_class_targets(ClassTargetParams P) {
  const long long n_in = (long long)P.B * P.D * P.H * P.W;
  const long long n_out = (long long)P.B * P.d * P.h * P.w * P.C;
  const long long in_per = (long long)P.D * P.H * P.W;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_in + n_out; i += (long long)gridDim.x * blockDim.x) {
    if (i >= n_out) {                                   // every label of the patch must be in the dict, sampled by the zoom or not
      const long long q = i - n_out;
      const int label = P.lab[q];
      if (label > 0 && class_code(P, (int)(q / in_per), label) == CODE_MISSING) atomicOr(P.missing, 1);
      continue;
    }
    const int c = (int)(i % P.C);
    long long p = i / P.C;
    float v = 0.f;
    if (P.neg && P.neg[p]) {
      v = -1.f;
    } else {
      const int x = (int)(p % P.w); p /= P.w;
      const int y = (int)(p % P.h); p /= P.h;
      const int z = (int)(p % P.d);
      const int b = (int)(p / P.d);
      const int sz = P.tz[z], sy = P.ty[y], sx = P.tx[x];
      if (sz >= 0 && sy >= 0 && sx >= 0) {
        const int label = max(P.lab[(((long long)b * P.D + sz) * P.H + sy) * P.W + sx], 0);      // (a negative id off the grid: background)
        const int code = class_code(P, b, label);
        if (c == 0) v = label == 0 ? 1.f : 0.f;
        else if (code == CODE_IGNORE) v = -1.f;
        else if (code == c) v = 1.f;
      }
    }
    P.out[i] = v;
  }
}

// ---- loss ---------------------------------------------------------------------------------------------------------------------
constexpr int LOSS_THREADS = 256;
constexpr int LOSS_PIX_PER_BLOCK = 4096;
constexpr double K_EPS = 1e-7;       // Keras' epsilon()

// One pixel per thread and round.  CMAX > 0: at most CMAX channels, exp(z - max) and the gradient w.r.t. the normalised probability held
// in registers; CMAX = 0: any channel count, both recomputed from the logits where they are needed (the same expressions).
//   p = softmax(z),  S = sum_c (p_c + e),  r = p / S,  q = clip(r, e, 1 - e),  L = -sum_c w_c [t_c >= 0] t_c log q_c
//   g_c = dL/dr_c = -w_c [t_c >= 0] t_c / q_c where e <= r_c <= 1 - e, else 0
//   a_j = dL/dp_j = g_j / S - (sum_c g_c p_c) / S^2            (p free: S depends on every p_j)
//   dL/dz_k = p_k (a_k - sum_j a_j p_j)
template <int CMAX>
__global__ __launch_bounds__(LOSS_THREADS) void k_class_loss(const float* __restrict__ logits, const float* __restrict__ target,
                                                             const double* __restrict__ weights, long long n_pix, int C, double scale,
                                                             double* __restrict__ part, float* __restrict__ dlogits) {
  constexpr int NR = CMAX ? CMAX : 1;
  const int n_c = CMAX ? CMAX : C;
  __shared__ double sh[LOSS_THREADS];
  double acc = 0.0;
  const long long p0 = (long long)blockIdx.x * LOSS_PIX_PER_BLOCK;
  const long long p1 = min(n_pix, p0 + LOSS_PIX_PER_BLOCK);
  for (long long pix = p0 + threadIdx.x; pix < p1; pix += LOSS_THREADS) {
    const float* z = logits + pix * C;
    const float* t = target + pix * C;
    double e[NR], g[NR];
    double m = (double)z[0];
    for (int c = 1; c < C; ++c) m = fmax(m, (double)z[c]);
    auto E = [&](int c) -> double {
      if constexpr (CMAX > 0) return e[c]; else return exp((double)z[c] - m);
    };
    double Z = 0.0;
#pragma unroll
    for (int c = 0; c < n_c; ++c)
      if (c < C) {
        const double v = exp((double)z[c] - m);
        if constexpr (CMAX > 0) e[c] = v;
        Z += v;
      }
    double S = 0.0;
#pragma unroll
    for (int c = 0; c < n_c; ++c)
      if (c < C) S += E(c) / Z + K_EPS;
    // dL/dr_c, and the pixel's loss term of the channel added to *loss when loss is given
    auto G = [&](int c, double p, double* loss) -> double {
      const double tc = (double)t[c];
      if (!(tc >= 0)) return 0.0;
      const double r = p / S;
      const double q = fmin(fmax(r, K_EPS), 1.0 - K_EPS);
      const double wt = weights[c] * tc;
      if (loss) *loss -= wt * log(q);
      return (r >= K_EPS && r <= 1.0 - K_EPS) ? -wt / q : 0.0;
    };
    double L = 0.0, gp = 0.0;
#pragma unroll
    for (int c = 0; c < n_c; ++c)
      if (c < C) {
        const double p = E(c) / Z;
        const double gc = G(c, p, &L);
        if constexpr (CMAX > 0) g[c] = gc;
        gp += gc * p;
      }
    acc += L;
    if (dlogits) {
      const double gS = gp / (S * S);
      double ap = 0.0;
#pragma unroll
      for (int c = 0; c < n_c; ++c)
        if (c < C) {
          const double p = E(c) / Z;
          double gc;
          if constexpr (CMAX > 0) gc = g[c]; else gc = G(c, p, nullptr);
          ap += (gc / S - gS) * p;
        }
#pragma unroll
      for (int c = 0; c < n_c; ++c)
        if (c < C) {
          const double p = E(c) / Z;
          double gc;
          if constexpr (CMAX > 0) gc = g[c]; else gc = G(c, p, nullptr);
          dlogits[pix * C + c] = (float)(scale * p * ((gc / S - gS) - ap));
        }
    }
  }
  sh[threadIdx.x] = acc;
  __syncthreads();
  for (int s = LOSS_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sh[0];
}

// one thread: the block partials in block order -> {class loss (Keras' mean over every pixel), w_class * class loss}
__global__ void k_class_loss_finish(const double* __restrict__ part, int n_blocks, long long n_pix, double w_class, double* __restrict__ losses) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double s = 0.0;
  for (int b = 0; b < n_blocks; ++b) s += part[b];
  losses[0] = s / (double)n_pix;
  losses[1] = w_class * losses[0];
}

}  // namespace

extern "C" int sd_class_targets_device(const int32_t* d_labels, int B, int D, int H, int W, const int32_t* d_meta, const int32_t* d_keys,
                                       const int32_t* d_codes, const int32_t* d_tz, const int32_t* d_ty, const int32_t* d_tx, int d, int h, int w,
                                       const unsigned char* d_neg, int n_channels, float* d_out, int32_t* d_missing, void* stream_) {
  if (!d_labels || !d_meta || !d_codes || !d_tz || !d_ty || !d_tx || !d_out || !d_missing || B <= 0 || D <= 0 || H <= 0 || W <= 0 || d <= 0 ||
      h <= 0 || w <= 0 || n_channels < 2) {
    sd::set_error("sd_class_targets: labels, tables, output and flag given, positive sizes, n_classes + 1 >= 2 channels");
    return -1;
  }
  ClassTargetParams P;
  P.lab = d_labels; P.meta = d_meta; P.keys = d_keys; P.codes = d_codes; P.tz = d_tz; P.ty = d_ty; P.tx = d_tx; P.neg = d_neg;
  P.out = d_out; P.missing = d_missing;
  P.B = B; P.D = D; P.H = H; P.W = W; P.d = d; P.h = h; P.w = w; P.C = n_channels;
  const long long n = (long long)B * D * H * W + (long long)B * d * h * w * n_channels;
  long long blocks = (n + 255) / 256;
  if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(k_class_targets, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_, P);
  SD_LAUNCH_CHECK();
  return 0;
}

extern "C" int sd_class_loss_device(const float* d_logits, const float* d_target, const double* d_class_weights, long long n_pix, int n_channels,
                                    double w_class, double* d_losses, float* d_grad_logits, void* stream_) {
  hipStream_t s = (hipStream_t)stream_;
  if (!d_logits || !d_target || !d_class_weights || !d_losses || n_pix <= 0 || n_channels < 2 ||
      (n_pix + LOSS_PIX_PER_BLOCK - 1) / LOSS_PIX_PER_BLOCK > 0x7fffffffLL) {
    sd::set_error("sd_class_loss: logits, targets, class weights and d_losses given, positive sizes, n_classes + 1 >= 2 channels");
    return -1;
  }
  const int n_blocks = sd::div_up(n_pix, LOSS_PIX_PER_BLOCK);
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  double* part = A.take_n<double>((size_t)n_blocks);
  if (!part) return -1;
  const double scale = w_class / (double)n_pix;
#define SD_CLASS_LOSS(CMAX)                                                                                                         \
  hipLaunchKernelGGL(k_class_loss<CMAX>, dim3(n_blocks), dim3(LOSS_THREADS), 0, s, d_logits, d_target, d_class_weights, n_pix, n_channels, \
                     scale, part, d_grad_logits)
  if (n_channels <= 2) SD_CLASS_LOSS(2);
  else if (n_channels <= 4) SD_CLASS_LOSS(4);
  else if (n_channels <= 8) SD_CLASS_LOSS(8);
  else SD_CLASS_LOSS(0);
#undef SD_CLASS_LOSS
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_class_loss_finish, dim3(1), dim3(64), 0, s, part, n_blocks, n_pix, w_class, d_losses);
  SD_LAUNCH_CHECK();
  return 0;
}
