// label_contacts.hip -- the contact table of a label image on the device (stardist_amd.utils.label_contacts and the neighbour columns
// of measure_labels): which labels touch, and over how many pixel pairs.
//
//   sd_label_contacts_device   every unordered pair {a, b}, a < b, of labels with a contact, with its number of contacts, ascending
//
// The per-pixel and per-wave rules are csrc/label_contacts.h's, shared with the host harness of the tests; the tile is
// csrc/label_edit.h's.
//   k_contacts<false>  one workgroup of LE_THREADS per tile (a workgroup strides over the tiles where there are more than MAX_BLOCKS):
//                      the tile's labels with a halo of 1 in LDS, then a wave takes the tile's rows one after the other, a lane per
//                      pixel, and for every forward offset of the connectivity the lanes form the key of their contact.  Consecutive
//                      lanes with the same key -- a border that runs along x -- are one run: a ballot of the lanes whose key differs
//                      from their left neighbour's gives the heads, the distance to the next head the run's length.  This pass counts
//                      the runs with a key and takes the min / max of the labels.
//   k_contacts<true>   the same traversal, twice per tile: a wave counts the runs of its rows of the tile, takes that many slots with
//                      one atomic (none for a tile without a contact), and on the second walk every run head writes (key, length) at
//                      the wave's base + its rank among the wave's heads so far.
// Then a radix sort of the keys (min << bits(max id) | max: only the bits the largest id needs, at most 62) and a reduce-by-key, as in
// csrc/overlap.hip.  All arithmetic is integer: the table does not depend on the order the runs arrive.  Two reads of the labels (the
// halo cells again, from cache), 16 bytes written and 64 sorted per run.  Untuned: the tile's back halo (the row above, the plane
// before) is loaded though no forward offset reads it; a row inside an object still walks every offset; the append pass walks a tile
// twice, which trades LDS reads for atomics on the one counter; the generic tile shape per rank.
#include "common.h"
#include "label_contacts.h"
#include "stardist_hip.h"
#include <hipcub/hipcub.hpp>
#include <limits.h>
#include <algorithm>

using namespace label_edit;
using namespace label_contacts;

namespace {

enum { PER_THREAD = LE_TILE_PIXELS / LE_THREADS, MAX_BLOCKS = 8192, MAX_EXTENT = INT_MAX - 2 * LE_TILE_X };

__global__ void k_contacts_init(unsigned long long* counter, int* mm) {
  if (threadIdx.x == 0) { *counter = 0; mm[0] = INT_MAX; mm[1] = INT_MIN; }
}

// The rows of a tile that this wave owns, one after the other, and for each the forward offsets of the connectivity: f(key, head,
// emits) is called by ALL 64 lanes for every row and offset that has a run with a key -- key: the lane's key or LC_NO_KEY, head: the
// lane starts a run, emits: the ballot of the lanes that start a run with a key.  lz and ly are the same for the whole wave (lx is the
// lane), so every branch around the shuffle and the ballot is uniform.
template <typename F>
__device__ __forceinline__ void each_row_and_offset(const int* cells, const Tile& g, const Origin& o, int connectivity, int with_background, int bits,
                                                    int lane, F f) {
  const int n_codes = code_count(g);
  for (int k = 0; k < PER_THREAD; ++k) {
    int lz, ly, lx;
    local_coords(g, k * LE_THREADS + (int)threadIdx.x, lz, ly, lx);
    if (!in_image(g, o, lz, ly, 0)) continue;                               // the row lies outside the image: the whole wave leaves
    for (int code = LC_FIRST_CODE; code < n_codes; ++code) {
      const Offset off = offset_of(code);
      if (off.moved > connectivity) continue;
      const unsigned long long key = contact_key(cells, g, o, lz, ly, lx, off, with_background, bits);
      const unsigned long long before = __shfl_up(key, 1);
      const bool head = run_head(key, before, lane);
      const unsigned long long emits = __ballot(head && key != LC_NO_KEY);
      if (emits) f(key, head, emits);
    }
  }
}

// WRITE = false: count the runs, min / max of the labels (bits: any value that keeps the keys apart, 32).  WRITE = true: append them; a
// wave first counts the runs of its rows of the tile, takes that many slots with one atomic, and fills them on a second walk.
template <bool WRITE>
__global__ void __launch_bounds__(LE_THREADS) k_contacts(const int* __restrict__ lbl, Tile g, long long tiles, int connectivity, int with_background,
                                                         int bits, unsigned long long* __restrict__ counter, int* __restrict__ mm, long long cap,
                                                         unsigned long long* __restrict__ keys, long long* __restrict__ lens) {
  __shared__ int cells[LE_LDS_CELLS];
  const int n_cells = cell_count(g);
  const int lane = (int)threadIdx.x & (LC_WAVE - 1);
  unsigned long long cnt = 0;                                               // the same in every lane of the wave
  int mn = INT_MAX, mx = INT_MIN;
  // a block takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ...: the same tiles for all its threads, so the barriers are uniform
  for (long long t = blockIdx.x; t < tiles; t += gridDim.x) {
    const Origin o = tile_origin(g, t);
    for (int c = (int)threadIdx.x; c < n_cells; c += LE_THREADS) {
      const int v = lbl[cell_source(g, o, c)];                              // every pixel is some tile's cell: the extrema need no test
      cells[c] = v;
      if (!WRITE) { mn = min(mn, v); mx = max(mx, v); }
    }
    __syncthreads();
    unsigned tile_runs = 0;
    each_row_and_offset(cells, g, o, connectivity, with_background, bits, lane,
                        [&](unsigned long long, bool, unsigned long long emits) { tile_runs += (unsigned)bit_count(emits); });
    if (!WRITE) {
      cnt += tile_runs;
    } else if (tile_runs) {                                                 // uniform
      unsigned long long base = 0;
      if (lane == 0) base = atomicAdd(counter, (unsigned long long)tile_runs);
      base = __shfl(base, 0);
      each_row_and_offset(cells, g, o, connectivity, with_background, bits, lane, [&](unsigned long long key, bool head, unsigned long long emits) {
        const unsigned long long heads = __ballot(head);
        const long long slot = (long long)base + run_slot(emits, lane);
        if (head && key != LC_NO_KEY && slot < cap) {
          keys[slot] = key;
          lens[slot] = run_length(heads, lane);
        }
        base += (unsigned)bit_count(emits);
      });
    }
    __syncthreads();                                                        // the next tile overwrites the cells
  }
  if (WRITE) return;
  for (int s = 32; s > 0; s >>= 1) {
    mn = min(mn, __shfl_xor(mn, s));
    mx = max(mx, __shfl_xor(mx, s));
  }
  if (lane == 0) {
    if (cnt) atomicAdd(counter, cnt);
    if (mn <= mx) { atomicMin(mm + 0, mn); atomicMax(mm + 1, mx); }
  }
}

__global__ void k_contacts_unpack(const unsigned long long* __restrict__ ckeys, const long long* __restrict__ sums, long long m, int bits,
                                  long long* __restrict__ okeys, long long* __restrict__ ocounts) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  okeys[i] = unpacked_key(ckeys[i], bits);
  ocounts[i] = sums[i];
}

}  // namespace

extern "C" int sd_label_contacts_device(const int32_t* d_lbl, int ndim, int Z, int Y, int X, int connectivity, int with_background, long long cap,
                                        int64_t* d_keys, int64_t* d_counts, long long* h_count, int32_t* h_minmax, long long* h_runs,
                                        void* stream) {
  hipStream_t s = (hipStream_t)stream;
  const char* who = "sd_label_contacts";
  if (!h_count || !h_minmax) { sd::set_error("%s: h_count and h_minmax are required", who); return -1; }
  *h_count = 0;
  h_minmax[0] = h_minmax[1] = 0;
  if (h_runs) *h_runs = 0;
  if ((ndim != 2 && ndim != 3) || (ndim == 2 && Z != 1)) { sd::set_error("%s: ndim must be 2 (with Z = 1) or 3", who); return -1; }
  if (connectivity < 1 || connectivity > ndim) { sd::set_error("%s: connectivity outside 1 .. %d", who, ndim); return -1; }
  if (cap < 0 || (cap > 0 && (!d_keys || !d_counts))) { sd::set_error("%s: bad output capacity / buffers", who); return -1; }
  if (Z <= 0 || Y <= 0 || X <= 0) return 0;
  if (!d_lbl) { sd::set_error("%s: null label image", who); return -1; }
  if (Z > MAX_EXTENT || Y > MAX_EXTENT || X > MAX_EXTENT) { sd::set_error("%s: an extent beyond 2^31 - 1 - %d", who, 2 * LE_TILE_X); return -1; }
  const Tile g = tile_of(Z, Y, X);
  const long long tiles = tile_count(g);
  const unsigned blocks = (unsigned)std::min<long long>(tiles, MAX_BLOCKS);
  sd::Arena& A = sd::arena();
  if (A.begin(s)) return -1;
  unsigned long long* counter = A.take_n<unsigned long long>(1);
  int* mm = A.take_n<int>(2);
  if (!counter || !mm) return -1;
  hipLaunchKernelGGL(k_contacts_init, dim3(1), dim3(64), 0, s, counter, mm);
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_contacts<false>, dim3(blocks), dim3(LE_THREADS), 0, s, (const int*)d_lbl, g, tiles, connectivity, with_background ? 1 : 0, 32,
                     counter, mm, 0ll, (unsigned long long*)nullptr, (long long*)nullptr);
  SD_LAUNCH_CHECK();
  unsigned long long runs = 0;
  SD_CHECK(hipMemcpyAsync(&runs, counter, sizeof(runs), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipMemcpyAsync(h_minmax, mm, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  if (h_minmax[0] < 0 || runs == 0) return 0;                        // negative labels: the caller raises; no contact
  if (runs > (unsigned long long)INT_MAX) { sd::set_error("%s: %llu runs exceed the sort's 2^31 - 1 items", who, runs); return -1; }
  const int R = (int)runs;
  const int bits = bits_of(h_minmax[1]);
  const int endBit = 2 * bits;                                       // <= 62
  unsigned long long* k0 = A.take_n<unsigned long long>(R);
  unsigned long long* k1 = A.take_n<unsigned long long>(R);
  long long* v0 = A.take_n<long long>(R);
  long long* v1 = A.take_n<long long>(R);
  int* nUnique = A.take_n<int>(1);
  size_t sortBytes = 0, redBytes = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sortBytes, k0, k1, v0, v1, R, 0, endBit, s);
  (void)hipcub::DeviceReduce::ReduceByKey(nullptr, redBytes, k1, k0, v1, v0, nUnique, hipcub::Sum(), R, s);
  void* tmp = A.take(std::max(sortBytes, redBytes) + 256);
  if (!k0 || !k1 || !v0 || !v1 || !nUnique || !tmp) return -1;
  SD_CHECK(hipMemsetAsync(counter, 0, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(k_contacts<true>, dim3(blocks), dim3(LE_THREADS), 0, s, (const int*)d_lbl, g, tiles, connectivity, with_background ? 1 : 0, bits,
                     counter, mm, (long long)R, k0, v0);
  SD_LAUNCH_CHECK();
  SD_CHECK(hipcub::DeviceRadixSort::SortPairs(tmp, sortBytes, k0, k1, v0, v1, R, 0, endBit, s));
  SD_CHECK(hipcub::DeviceReduce::ReduceByKey(tmp, redBytes, k1, k0, v1, v0, nUnique, hipcub::Sum(), R, s));
  int m = 0;
  unsigned long long written = 0;
  SD_CHECK(hipMemcpyAsync(&m, nUnique, sizeof(int), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipMemcpyAsync(&written, counter, sizeof(written), hipMemcpyDeviceToHost, s));
  SD_CHECK(hipStreamSynchronize(s));
  if (written != runs) { sd::set_error("%s: the two passes found %llu and %llu runs", who, runs, written); return -1; }
  *h_count = m;
  if (h_runs) *h_runs = (long long)runs;
  const long long w = std::min<long long>(m, cap);
  if (w > 0) {
    hipLaunchKernelGGL(k_contacts_unpack, dim3((unsigned)((w + 255) / 256)), dim3(256), 0, s, (const unsigned long long*)k0, (const long long*)v0, w,
                       bits, (long long*)d_keys, (long long*)d_counts);
    SD_LAUNCH_CHECK();
  }
  return 0;
}
