// relabel.hip -- relabel a stack of label images through one (raw id -> new id) table per frame (the repaint loop of
// stardist/matching.py:452-465 for all frames at once).
//
//   sd_relabel_stack_device   out[k][i] = new id of ys[k][i]; 0 stays 0
//
// A frame whose largest id is small gets a dense table (new id at index raw id, built here from the sorted list); a frame with large,
// sparse ids is served by a binary search in its sorted ids.  One launch covers the stack: 16-byte loads and stores, a lane keeps its
// last lookup (neighbouring pixels mostly carry the same id).
#include "common.h"
#include "../../include/stardist_hip.h"
#include <limits.h>
#include <algorithm>
#include <vector>

namespace {

enum { BLOCK = 256, MAX_BLOCKS_X = 8192, MAX_FRAMES_Y = 65535 };
const int DENSE_MAX_ID = (1 << 22) - 1;              // a dense table of at most 16 MiB per frame ...
const long long DENSE_TOTAL = 1ll << 26;             // ... and 256 MiB per call; frames beyond either are searched

struct FrameTab {
  long long idOff;       // first entry of the frame in ids / news
  long long tabOff;      // first entry of its dense table, -1: search
  int count, maxId;
};

__global__ void k_fill_tables(const FrameTab* __restrict__ ft, int K, const int* __restrict__ ids, const int* __restrict__ news,
                              int* __restrict__ tab) {
  for (int k = blockIdx.y; k < K; k += gridDim.y) {
    const FrameTab f = ft[k];
    if (f.tabOff < 0) continue;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < f.count; i += (long long)gridDim.x * blockDim.x) {
      const int id = ids[f.idOff + i];
      if (id > 0 && id <= f.maxId) tab[f.tabOff + id] = news[f.idOff + i];
    }
  }
}

__device__ __forceinline__ int lookup(const FrameTab& f, const int* __restrict__ ids, const int* __restrict__ news, const int* __restrict__ tab,
                                      int y, int& lastY, int& lastV) {
  if (y == lastY) return lastV;
  int v = 0;
  if (y > 0 && y <= f.maxId) {
    if (f.tabOff >= 0) {
      v = tab[f.tabOff + y];
    } else {
      int lo = 0, hi = f.count;                      // first entry >= y
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (ids[f.idOff + mid] < y) lo = mid + 1; else hi = mid;
      }
      if (lo < f.count && ids[f.idOff + lo] == y) v = news[f.idOff + lo];
    }
  }
  lastY = y; lastV = v;
  return v;
}

__global__ void __launch_bounds__(BLOCK) k_relabel_stack(const int* __restrict__ ys, int K, long long n, bool vec, const FrameTab* __restrict__ ft,
                                                         const int* __restrict__ ids, const int* __restrict__ news, const int* __restrict__ tab,
                                                         int* __restrict__ out) {
  const long long nQuads = (n + 3) / 4;
  for (int k = blockIdx.y; k < K; k += gridDim.y) {
    const FrameTab f = ft[k];
    const int* __restrict__ y = ys + (long long)k * n;
    int* __restrict__ o = out + (long long)k * n;
    int lastY = 0, lastV = 0;
    for (long long q = (long long)blockIdx.x * BLOCK + threadIdx.x; q < nQuads; q += (long long)gridDim.x * BLOCK) {
      const long long i0 = q * 4;
      if (vec) {
        const int4 a = *reinterpret_cast<const int4*>(y + i0);
        int4 r;
        r.x = lookup(f, ids, news, tab, a.x, lastY, lastV);
        r.y = lookup(f, ids, news, tab, a.y, lastY, lastV);
        r.z = lookup(f, ids, news, tab, a.z, lastY, lastV);
        r.w = lookup(f, ids, news, tab, a.w, lastY, lastV);
        *reinterpret_cast<int4*>(o + i0) = r;
      } else {
        const int v = (int)min(4ll, n - i0);
        for (int j = 0; j < v; ++j) o[i0 + j] = lookup(f, ids, news, tab, y[i0 + j], lastY, lastV);
      }
    }
  }
}

}  // namespace

extern "C" int sd_relabel_stack_device(const int32_t* d_ys, int K, long long n, const int32_t* d_ids, const int32_t* d_new,
                                       const long long* h_offsets, const int32_t* h_max, int32_t* d_out, void* stream) {
  hipStream_t s = (hipStream_t)stream;
  if (K <= 0 || n <= 0) return 0;
  if (!d_ys || !d_out || !h_offsets || !h_max) { sd::set_error("sd_relabel_stack: ys, out, h_offsets and h_max are required"); return -1; }
  std::vector<FrameTab> ft(K);
  long long tabTotal = 0;
  for (int k = 0; k < K; ++k) {
    const long long c = h_offsets[k + 1] - h_offsets[k];
    if (h_offsets[k] < 0 || c < 0 || c > INT_MAX || h_max[k] < 0 || (c > 0 && (!d_ids || !d_new))) {
      sd::set_error("sd_relabel_stack: bad table of frame %d", k);
      return -1;
    }
    ft[k].idOff = h_offsets[k];
    ft[k].count = (int)c;
    ft[k].maxId = h_max[k];
    ft[k].tabOff = -1;
    if (c > 0 && h_max[k] <= DENSE_MAX_ID && tabTotal + h_max[k] + 1 <= DENSE_TOTAL) {
      ft[k].tabOff = tabTotal;
      tabTotal += ((long long)h_max[k] + 1 + 3) & ~3ll;
    }
  }
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  FrameTab* dft = A.take_n<FrameTab>(K);
  int* tab = A.take_n<int>((size_t)tabTotal);
  if (!dft || !tab) return -1;
  SD_CHECK(hipMemcpyAsync(dft, ft.data(), (size_t)K * sizeof(FrameTab), hipMemcpyHostToDevice, s));
  SD_CHECK(hipStreamSynchronize(s));                                    // ft leaves scope with this call
  const int gy = std::min(K, (int)MAX_FRAMES_Y);
  if (tabTotal > 0) {
    SD_CHECK(hipMemsetAsync(tab, 0, (size_t)tabTotal * sizeof(int), s));
    int maxCount = 1;
    for (int k = 0; k < K; ++k) maxCount = std::max(maxCount, ft[k].count);
    hipLaunchKernelGGL(k_fill_tables, dim3(std::min((maxCount + BLOCK - 1) / BLOCK, 1024), gy), dim3(BLOCK), 0, s, (const FrameTab*)dft, K,
                       (const int*)d_ids, (const int*)d_new, tab);
    SD_LAUNCH_CHECK();
  }
  const long long nQuads = (n + 3) / 4;
  const bool vec = ((uintptr_t)d_ys % 16 == 0) && ((uintptr_t)d_out % 16 == 0) && (n % 4 == 0);
  const int gx = (int)std::min<long long>((nQuads + BLOCK - 1) / BLOCK, MAX_BLOCKS_X);
  hipLaunchKernelGGL(k_relabel_stack, dim3(gx, gy), dim3(BLOCK), 0, s, (const int*)d_ys, K, n, vec, (const FrameTab*)dft, (const int*)d_ids,
                     (const int*)d_new, (const int*)tab, d_out);
  SD_LAUNCH_CHECK();
  return 0;
}
