// train3d.hip -- the backward pass of StarDist3D training (stardist/models/model3d.py train; the U-Net and ResNet graphs of
// model3d.py:370-452): what the 2D backward (train2d.hip) does not already cover for the 3D shapes and the ResNet layers, and the
// max-pool and up-sampling adjoints of both models:
//
//   * k_wgrad3: weight gradient of a 3D convolution as a GEMM on the f32 matrix cores (v_mfma_f32_32x32x2_f32, exact f32 products)
//         dW[co][n] = sum_{b,zo,yo,xo} g[b][zo][yo][xo][co] * in[b][zo*sz - pz + dz][yo*sy - py + dy][xo*sx - px + dx][ci]
//     with M = c_out, N = n = (tap, ci) flattened (tap-major; c_in is not padded, so the one-channel 7x7x7 stem has 343 columns, not
//     343 x 32) and K = output voxels.  Any kernel size, stride and padding before the first element (the convention of
//     sd_convg_ndhwc_device); the input takes the forward kernels' two-source form [up-sampled src0 | src1] with up bits 1 (x), 2 (y),
//     4 (z), so the first convolution of a U-Net up level gets its gradient without the concatenation being written.
//     Partition: a workgroup owns (voxel-row chunk, 32 output channels, 128 columns); each of its four waves holds ONE 32 x 32
//     accumulator (16 floats per lane) for its 32 columns.  A 3x3x3 layer's 27 taps thus spread over the waves and workgroups of the
//     column axis instead of living in one wave (27 x 16 accumulators would need 432 of the 512 VGPR + AGPR per lane).  The operands
//     are read straight from global memory, one voxel pair per MFMA (the lane half picks the voxel); a tap's input rows are re-read
//     from L2 by the columns of the other taps -- the price of the small register footprint, which keeps many waves per SIMD.
//     The output rows (b, zo, yo) are split into chunks that depend on the shape only; each chunk writes its partial sums to the
//     workspace and k_wgrad3_reduce adds them in chunk order in float64.  No atomics: two calls give the same bits.
//   * k_dgrad3: data gradient of a strided convolution (the transposed convolution), one thread per input element:
//         gin[b][z][y][x][ci] = sum_{taps, in order} sum_{co, ascending} g[b][zo][yo][xo][co] * w[co][ci][dz][dy][dx]
//     over the taps with z = zo*sz - pz + dz (etc.) for an output voxel inside the output -- one fixed f32 fma chain per element.
//     The stride-1 3x3x3 layers do not come here: their data gradient is the forward kernel on the flipped, transposed kernel.
//   * k_maxpool3_adjoint, k_upcat3_adjoint: the adjoints of MaxPooling (first maximum of each window in scan order z, y, x) and
//     UpSampling + Concatenate (a fixed-order sum over each window: dz, dy, dx), for both models: the 2D entry points
//     (sd_maxpool_adjoint_ndhwc_device, sd_upcat_adjoint_ndhwc_device) check their own arguments and run these kernels with D = 1.
//
// The losses are those of the 2D model (stardist/models/base.py:34-60, 315-325 -- the 3D model compiles the same ones): the 3D step
// calls sd_stardist_loss2d_device of train2d.hip with n_pix = B * d * h * w, and there is no second loss kernel.
#include "common.h"
#include "stardist_hip.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int WG3_THREADS = 256;                 // 4 waves
constexpr int WG3_COLS = 128;                    // 32 columns per wave

struct Wgrad3Params {
  const float* g;          // [B][Do][Ho][Wo][c_out]
  const float* s0;         // [B][D >> z0][H >> y0][W >> x0][c0]
  const float* s1;         // [B][D >> z1][H >> y1][W >> x1][c1] (c1 == 0: unused)
  float* ws;               // [n_chunks][co_pad][n_pad]
  float* wsb;              // [n_chunks][co_pad] (bias partials)
  int c_out, c0, c1, z0, y0, x0, z1, y1, x1;
  int D, H, W, kz, ky, kx, sz, sy, sx, pz, py, px, Do, Ho, Wo;
  int n_cols, n_pad, co_pad, n_rows, rows_per_chunk;
};

__global__ __launch_bounds__(WG3_THREADS) void k_wgrad3(Wgrad3Params P) {
  const int chunk = blockIdx.x, cg = blockIdx.y, ng = blockIdx.z;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l32 = lane & 31, h = lane >> 5;
  const int c_in = P.c0 + P.c1;
  const int col0 = (ng * 4 + wave) * 32;           // the wave's first column (wave-uniform)
  const int col = col0 + l32;
  const bool col_ok = col < P.n_cols;
  const int t = col_ok ? col / c_in : 0, cia = col_ok ? col - t * c_in : 0;
  const int dz = t / (P.ky * P.kx), dy = (t / P.kx) % P.ky, dx = t % P.kx;
  const bool first = cia < P.c0;                   // the lane's source and channel in it
  const float* src = first ? P.s0 : P.s1;
  const int cs = first ? P.c0 : P.c1, ci = first ? cia : cia - P.c0;
  const int zs = first ? P.z0 : P.z1, ys = first ? P.y0 : P.y1, xs = first ? P.x0 : P.x1;
  const int Ds = P.D >> zs, Hs = P.H >> ys, Ws = P.W >> xs;
  const int co = cg * 32 + l32;
  const bool co_ok = co < P.c_out;
  const bool do_bias = ng == 0 && wave == 0;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float bsum = 0.f;
  const int r_begin = chunk * P.rows_per_chunk;
  const int r_end = min(P.n_rows, r_begin + P.rows_per_chunk);
  const int steps = (P.Wo + 1) >> 1;
  if (col0 < P.n_cols) {
    for (int r = r_begin; r < r_end; ++r) {
      const int oy = r % P.Ho, q = r / P.Ho;
      const int oz = q % P.Do, b = q / P.Do;
      const int iz = oz * P.sz - P.pz + dz, iy = oy * P.sy - P.py + dy;
      const bool row_ok = col_ok && iz >= 0 && iz < P.D && iy >= 0 && iy < P.H;
      const float* grow = P.g + (long long)r * P.Wo * P.c_out + co;
      const float* srow = row_ok ? src + (((long long)b * Ds + (iz >> zs)) * Hs + (iy >> ys)) * (long long)Ws * cs + ci : src;
      for (int s = 0; s < steps; ++s) {
        const int ox = 2 * s + h;
        const bool ok = ox < P.Wo;
        const float a = (ok && co_ok) ? grow[(long long)ox * P.c_out] : 0.f;
        const int ix = ox * P.sx - P.px + dx;
        const float bv = (ok && row_ok && ix >= 0 && ix < P.W) ? srow[(long long)(ix >> xs) * cs] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bv, acc, 0, 0, 0);
        bsum += a;
      }
    }
  }
  float* dst = P.ws + (size_t)chunk * P.co_pad * P.n_pad;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const int cr = cg * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
    dst[(size_t)cr * P.n_pad + col] = acc[q];
  }
  if (do_bias) {
    const float other = __shfl_down(bsum, 32);      // the odd voxels' sum (lane half 1) to lane half 0
    if (h == 0) P.wsb[(size_t)chunk * P.co_pad + co] = bsum + other;
  }
}

// dW[co][ci][tap] = sum over chunks (ascending) of the partials of column tap * c_in + ci; db[co] likewise
__global__ void k_wgrad3_reduce(const float* __restrict__ ws, const float* __restrict__ wsb, int n_chunks, int n_cols, int c_in, int c_out,
                                int co_pad, int n_pad, float* __restrict__ dw, float* __restrict__ db) {
  const long long n = (long long)c_out * n_cols;
  const size_t cstride = (size_t)co_pad * n_pad;
  const int taps = n_cols / c_in;
  for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < n + c_out; idx += (long long)gridDim.x * blockDim.x) {
    if (idx < n) {
      const int co = (int)(idx / n_cols), col = (int)(idx - (long long)co * n_cols);
      const int t = col / c_in, ci = col - t * c_in;
      const size_t off = (size_t)co * n_pad + col;
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

struct Dgrad3Params {
  const float* g;          // [B][Do][Ho][Wo][c_out]
  const float* wt;         // [kz][ky][kx][c_out][c_in]
  float* gin;              // [B][D][H][W][c_in]
  int c_out, c_in, D, H, W, kz, ky, kx, sz, sy, sx, pz, py, px, Do, Ho, Wo;
  long long n;
};

__global__ void k_dgrad3(Dgrad3Params P) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < P.n; i += (long long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % P.c_in);
    long long r = i / P.c_in;
    const int x = (int)(r % P.W); r /= P.W;
    const int y = (int)(r % P.H); r /= P.H;
    const int z = (int)(r % P.D);
    const long long b = r / P.D;
    float s = 0.f;
    for (int dz = 0; dz < P.kz; ++dz) {
      const int tz = z + P.pz - dz;
      if (tz < 0 || tz % P.sz) continue;
      const int oz = tz / P.sz;
      if (oz >= P.Do) continue;
      for (int dy = 0; dy < P.ky; ++dy) {
        const int ty = y + P.py - dy;
        if (ty < 0 || ty % P.sy) continue;
        const int oy = ty / P.sy;
        if (oy >= P.Ho) continue;
        for (int dx = 0; dx < P.kx; ++dx) {
          const int tx = x + P.px - dx;
          if (tx < 0 || tx % P.sx) continue;
          const int ox = tx / P.sx;
          if (ox >= P.Wo) continue;
          const float* gp = P.g + (((b * P.Do + oz) * P.Ho + oy) * (long long)P.Wo + ox) * P.c_out;
          const float* wp = P.wt + (size_t)((dz * P.ky + dy) * P.kx + dx) * P.c_out * P.c_in + ci;
          for (int co = 0; co < P.c_out; ++co) s = fmaf(gp[co], wp[(size_t)co * P.c_in], s);
        }
      }
    }
    P.gin[i] = s;
  }
}

// one thread per INPUT element: the gradient of its window's output goes to the window's first maximum (scan order z, y, x; a NaN
// counts as a maximum, as in torch's CPU max-pool); elements of a window that is not the maximum, and planes / rows / columns beyond
// the last whole window, get zero.  A 2D pooling is D = 1, pz = 1: the scan is y, x.
__global__ void k_maxpool3_adjoint(const float* __restrict__ x, const float* __restrict__ gout, int C, int D, int H, int W, int pz, int py,
                                   int px, long long n, float* __restrict__ gin) {
  const int Do = D / pz, Ho = H / py, Wo = W / px;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    long long r = i / C;
    const int xx = (int)(r % W); r /= W;
    const int yy = (int)(r % H); r /= H;
    const int zz = (int)(r % D);
    const long long b = r / D;
    const int oz = zz / pz, oy = yy / py, ox = xx / px;
    float v = 0.f;
    if (oz < Do && oy < Ho && ox < Wo) {
      int bz = oz * pz, by = oy * py, bx = ox * px;
      float m = x[(((b * D + bz) * H + by) * W + bx) * C + c];
      for (int dz = 0; dz < pz; ++dz)
        for (int dy = 0; dy < py; ++dy)
          for (int dx = 0; dx < px; ++dx) {
            const int z = oz * pz + dz, y = oy * py + dy, xq = ox * px + dx;
            const float u = x[(((b * D + z) * H + y) * W + xq) * C + c];
            if (u > m || (u != u && m == m)) { m = u; bz = z; by = y; bx = xq; }
          }
      if (bz == zz && by == yy && bx == xx) v = gout[(((b * Do + oz) * Ho + oy) * Wo + ox) * C + c];
    }
    gin[i] = v;
  }
}

// gcat [B][D][H][W][c0 + c1] -> g1 = its last c1 channels, g0 [B][D >> sz][H >> sy][W >> sx][c0] = the sum over each up-sampling
// window of its first c0 channels (window order: dz, dy, dx; 2D is D = 1, sz = 0: dy, dx)
__global__ void k_upcat3_adjoint(const float* __restrict__ gcat, int c0, int c1, int sz, int sy, int sx, int D, int H, int W, long long n0,
                                 long long n1, float* __restrict__ g0, float* __restrict__ g1) {
  const int C = c0 + c1, D0 = D >> sz, H0 = H >> sy, W0 = W >> sx;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n0 + n1; i += (long long)gridDim.x * blockDim.x) {
    if (i < n0) {
      const int c = (int)(i % c0);
      long long r = i / c0;
      const int x = (int)(r % W0); r /= W0;
      const int y = (int)(r % H0); r /= H0;
      const int z = (int)(r % D0);
      const long long b = r / D0;
      float s = 0.f;
      for (int dz = 0; dz <= sz; ++dz)
        for (int dy = 0; dy <= sy; ++dy)
          for (int dx = 0; dx <= sx; ++dx)
            s += gcat[(((b * D + (z << sz) + dz) * H + (y << sy) + dy) * W + (x << sx) + dx) * C + c];
      g0[i] = s;
    } else {
      const long long j = i - n0;
      const int c = (int)(j % c1);
      g1[j] = gcat[(j / c1) * C + c0 + c];
    }
  }
}

inline unsigned grid_for(long long n, int threads = 256) {
  long long b = (n + threads - 1) / threads;
  return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

int wgrad3_launch(Wgrad3Params P, int B, float* d_dw, float* d_db, hipStream_t s) {
  const int c_in = P.c0 + P.c1;
  const int taps = P.kz * P.ky * P.kx;
  P.n_cols = taps * c_in;
  const int n_groups = sd::div_up(P.n_cols, WG3_COLS), co_groups = sd::div_up(P.c_out, 32);
  P.n_pad = n_groups * WG3_COLS;
  P.co_pad = co_groups * 32;
  P.n_rows = B * P.Do * P.Ho;
  // the row chunks: a function of the shape only (about 2048 workgroups, at most 2^24 partial floats)
  const long long per_chunk = (long long)P.co_pad * P.n_pad;
  long long n_chunks = sd::div_up(2048, (long long)co_groups * n_groups);
  const long long cap = (1LL << 24) / per_chunk;
  if (n_chunks > cap) n_chunks = cap;
  if (n_chunks < 1) n_chunks = 1;
  if (n_chunks > P.n_rows) n_chunks = P.n_rows;
  P.rows_per_chunk = (int)sd::div_up((long long)P.n_rows, n_chunks);
  n_chunks = sd::div_up((long long)P.n_rows, (long long)P.rows_per_chunk);
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  P.ws = A.take_n<float>((size_t)n_chunks * per_chunk);
  P.wsb = A.take_n<float>((size_t)n_chunks * P.co_pad);
  if (!P.ws || !P.wsb) return -1;
  hipLaunchKernelGGL(k_wgrad3, dim3((unsigned)n_chunks, (unsigned)co_groups, (unsigned)n_groups), dim3(WG3_THREADS), 0, s, P);
  SD_LAUNCH_CHECK();
  const long long n = (long long)P.c_out * P.n_cols + P.c_out;
  hipLaunchKernelGGL(k_wgrad3_reduce, dim3(grid_for(n)), dim3(256), 0, s, P.ws, P.wsb, (int)n_chunks, P.n_cols, c_in, P.c_out, P.co_pad,
                     P.n_pad, d_dw, d_db);
  SD_LAUNCH_CHECK();
  return 0;
}

bool bad_up(int up, int D, int H, int W) {
  return (up & ~7) || ((up & 1) && (W & 1)) || ((up & 2) && (H & 1)) || ((up & 4) && (D & 1));
}

}  // namespace

extern "C" int sd_conv3_wgrad_ndhwc_device(const float* d_g, int c_out, const float* d_src0, int c0, int up0, const float* d_src1, int c1,
                                           int up1, int B, int D, int H, int W, float* d_dw, float* d_db, void* stream_) {
  if (!d_g || !d_src0 || !d_dw || c_out <= 0 || c0 <= 0 || c1 < 0 || (c1 > 0 && !d_src1) || B <= 0 || D <= 0 || H <= 0 || W <= 0 ||
      bad_up(up0, D, H, W) || (c1 > 0 && bad_up(up1, D, H, W)) || (long long)27 * (c0 + c1) > (1 << 30)) {
    sd::set_error("sd_conv3_wgrad_ndhwc: up bits 1 (x) / 2 (y) / 4 (z) over even sizes, positive sizes");
    return -1;
  }
  Wgrad3Params P;
  P.g = d_g; P.s0 = d_src0; P.s1 = c1 > 0 ? d_src1 : nullptr; P.c_out = c_out; P.c0 = c0; P.c1 = c1;
  P.x0 = up0 & 1; P.y0 = (up0 >> 1) & 1; P.z0 = (up0 >> 2) & 1;
  P.x1 = c1 > 0 ? (up1 & 1) : 0; P.y1 = c1 > 0 ? ((up1 >> 1) & 1) : 0; P.z1 = c1 > 0 ? ((up1 >> 2) & 1) : 0;
  P.D = D; P.H = H; P.W = W; P.kz = P.ky = P.kx = 3; P.sz = P.sy = P.sx = 1; P.pz = P.py = P.px = 1;
  P.Do = D; P.Ho = H; P.Wo = W;
  return wgrad3_launch(P, B, d_dw, d_db, (hipStream_t)stream_);
}

extern "C" int sd_convg_wgrad_ndhwc_device(const float* d_g, int c_out, const float* d_src, int c_in, int B, int D, int H, int W, int kz, int ky,
                                           int kx, int sz, int sy, int sx, int pz, int py, int px, int Do, int Ho, int Wo, float* d_dw,
                                           float* d_db, void* stream_) {
  if (!d_g || !d_src || !d_dw || c_out <= 0 || c_in <= 0 || B <= 0 || D <= 0 || H <= 0 || W <= 0 || kz <= 0 || ky <= 0 || kx <= 0 ||
      sz <= 0 || sy <= 0 || sx <= 0 || pz < 0 || py < 0 || px < 0 || Do <= 0 || Ho <= 0 || Wo <= 0 ||
      (long long)kz * ky * kx * c_in > (1 << 30)) {
    sd::set_error("sd_convg_wgrad_ndhwc: positive sizes, kernel and strides, non-negative padding");
    return -1;
  }
  Wgrad3Params P;
  P.g = d_g; P.s0 = d_src; P.s1 = nullptr; P.c_out = c_out; P.c0 = c_in; P.c1 = 0;
  P.x0 = P.y0 = P.z0 = P.x1 = P.y1 = P.z1 = 0;
  P.D = D; P.H = H; P.W = W; P.kz = kz; P.ky = ky; P.kx = kx; P.sz = sz; P.sy = sy; P.sx = sx; P.pz = pz; P.py = py; P.px = px;
  P.Do = Do; P.Ho = Ho; P.Wo = Wo;
  return wgrad3_launch(P, B, d_dw, d_db, (hipStream_t)stream_);
}

extern "C" int sd_convg_dgrad_ndhwc_device(const float* d_g, int c_out, const float* d_wt, int c_in, int B, int D, int H, int W, int kz, int ky,
                                           int kx, int sz, int sy, int sx, int pz, int py, int px, int Do, int Ho, int Wo, float* d_gin,
                                           void* stream_) {
  if (!d_g || !d_wt || !d_gin || c_out <= 0 || c_in <= 0 || B < 0 || D < 0 || H < 0 || W < 0 || kz <= 0 || ky <= 0 || kx <= 0 || sz <= 0 ||
      sy <= 0 || sx <= 0 || pz < 0 || py < 0 || px < 0 || Do <= 0 || Ho <= 0 || Wo <= 0) {
    sd::set_error("sd_convg_dgrad_ndhwc: positive sizes, kernel and strides, non-negative padding");
    return -1;
  }
  Dgrad3Params P;
  P.g = d_g; P.wt = d_wt; P.gin = d_gin; P.c_out = c_out; P.c_in = c_in; P.D = D; P.H = H; P.W = W;
  P.kz = kz; P.ky = ky; P.kx = kx; P.sz = sz; P.sy = sy; P.sx = sx; P.pz = pz; P.py = py; P.px = px; P.Do = Do; P.Ho = Ho; P.Wo = Wo;
  P.n = (long long)B * D * H * W * c_in;
  if (P.n == 0) return 0;
  hipLaunchKernelGGL(k_dgrad3, dim3(grid_for(P.n)), dim3(256), 0, (hipStream_t)stream_, P);
  SD_LAUNCH_CHECK();
  return 0;
}

extern "C" int sd_maxpool3d_adjoint_ndhwc_device(const float* d_in, const float* d_gout, int n_channels, int B, int D, int H, int W, int pz,
                                                 int py, int px, float* d_gin, void* stream_) {
  if (!d_in || !d_gout || !d_gin || n_channels <= 0 || B < 0 || D < 0 || H < 0 || W < 0 || pz < 1 || py < 1 || px < 1) {
    sd::set_error("sd_maxpool3d_adjoint_ndhwc: invalid arguments");
    return -1;
  }
  const long long n = (long long)B * D * H * W * n_channels;
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_maxpool3_adjoint, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream_, d_in, d_gout, n_channels, D, H, W, pz, py, px,
                     n, d_gin);
  SD_LAUNCH_CHECK();
  return 0;
}

extern "C" int sd_upcat3d_adjoint_ndhwc_device(const float* d_gcat, int c0, int up0, int c1, int B, int D, int H, int W, float* d_g0,
                                               float* d_g1, void* stream_) {
  if (!d_gcat || !d_g0 || c0 <= 0 || c1 < 0 || (c1 > 0 && !d_g1) || B < 0 || D < 0 || H < 0 || W < 0 || bad_up(up0, D, H, W)) {
    sd::set_error("sd_upcat3d_adjoint_ndhwc: up bits 1 (x) / 2 (y) / 4 (z) over even sizes");
    return -1;
  }
  const int sx = up0 & 1, sy = (up0 >> 1) & 1, sz = (up0 >> 2) & 1;
  const long long n0 = (long long)B * (D >> sz) * (H >> sy) * (W >> sx) * c0, n1 = (long long)B * D * H * W * c1;
  if (n0 + n1 == 0) return 0;
  hipLaunchKernelGGL(k_upcat3_adjoint, dim3(grid_for(n0 + n1)), dim3(256), 0, (hipStream_t)stream_, d_gcat, c0, c1, sz, sy, sx, D, H, W, n0, n1,
                     d_g0, d_g1);
  SD_LAUNCH_CHECK();
  return 0;
}

// the 2D adjoints: the 3D kernels on one plane per sample (D = 1, pz = 1, up bit 4 clear)
extern "C" int sd_maxpool_adjoint_ndhwc_device(const float* d_in, const float* d_gout, int n_channels, int B, int H, int W, int py, int px,
                                               float* d_gin, void* stream_) {
  if (!d_in || !d_gout || !d_gin || n_channels <= 0 || B < 0 || H < 0 || W < 0 || py < 1 || px < 1) {
    sd::set_error("sd_maxpool_adjoint_ndhwc: invalid arguments");
    return -1;
  }
  return sd_maxpool3d_adjoint_ndhwc_device(d_in, d_gout, n_channels, B, 1, H, W, 1, py, px, d_gin, stream_);
}

extern "C" int sd_upcat_adjoint_ndhwc_device(const float* d_gcat, int c0, int up0, int c1, int B, int H, int W, float* d_g0, float* d_g1,
                                             void* stream_) {
  if (!d_gcat || !d_g0 || c0 <= 0 || c1 < 0 || (c1 > 0 && !d_g1) || B < 0 || H < 0 || W < 0 || (up0 & ~3) || ((up0 & 1) && (W & 1)) ||
      ((up0 & 2) && (H & 1))) {
    sd::set_error("sd_upcat_adjoint_ndhwc: up bits 1 (x) / 2 (y) over even sizes");
    return -1;
  }
  return sd_upcat3d_adjoint_ndhwc_device(d_gcat, c0, up0, c1, B, 1, H, W, d_g0, d_g1, stream_);
}
