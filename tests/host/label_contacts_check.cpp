// label_contacts_check.cpp -- the per-pixel and per-wave rules of stardist_amd/csrc/label_contacts.h on the host, in the order the
// kernels of csrc/label_contacts.hip visit the pixels: tile after tile with the tile's cells in a local array, row after row, offset
// after offset, the 64 lanes of a wave as an array.  A stand-alone program: it reads the records tests/test_cpu_label_contacts.py wrote
// (inputs and the host route's tables), recomputes every table -- a count pass, an append pass, a sort and a reduce-by-key -- in two
// orders of the tiles, and compares.  It is built plain and under the address and undefined-behaviour sanitizers.
//
//   label_contacts_check <records file>      prints "<n> records, <bad> bad"; exit status 0 only with 0 bad
//
// A record: int32 ndim, Z, Y, X, connectivity, with_background; int64 m, spare; int32 lbl[Z * Y * X]; int64 keys[m] (a << 32 | b);
// int64 counts[m].
#include "../../stardist_amd/csrc/label_contacts.h"

#include <limits.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <utility>
#include <vector>

using namespace label_edit;
using namespace label_contacts;

typedef std::vector<std::pair<unsigned long long, long long> > Runs;

// one pass of k_contacts over the tiles in the given order: the number of runs with a key; with `out`, the runs appended at the slots
// the kernel would give them (a wave's base + the rank of the run among the wave's runs).  -2: a rule broke an invariant
static long long pass(const int* lbl, const Tile& g, bool reversed, int connectivity, int with_background, int bits, Runs* out, int* mn, int* mx) {
  std::vector<int> cells(LE_LDS_CELLS);
  if (cell_count(g) > (int)LE_LDS_CELLS) return -2;
  long long count = 0;
  const long long tiles = tile_count(g);
  for (long long i = 0; i < tiles; ++i) {
    const long long t = reversed ? tiles - 1 - i : i;
    const Origin o = tile_origin(g, t);
    cells.assign(LE_LDS_CELLS, INT_MIN);                                   // a cell that is read without having been loaded shows
    for (int c = 0; c < cell_count(g); ++c) cells[c] = lbl[cell_source(g, o, c)];
    for (int row = 0; row < LE_TILE_PIXELS / LC_WAVE; ++row) {              // a wave and one of its LE_TILE_PIXELS / LE_THREADS rows
      int lz, ly, lx;
      local_coords(g, row * LC_WAVE, lz, ly, lx);
      if (lz >= g.tz || !in_image(g, o, lz, ly, 0)) continue;
      for (int lane = 0; lane < LC_WAVE; ++lane) {
        if (!in_image(g, o, lz, ly, lane)) continue;
        const int v = cells[((lz + g.hz) * g.cy + (ly + 1)) * g.cx + (lane + 1)];
        *mn = std::min(*mn, v); *mx = std::max(*mx, v);
      }
      for (int code = LC_FIRST_CODE; code < code_count(g); ++code) {
        const Offset off = offset_of(code);
        if (off.moved > connectivity) continue;
        unsigned long long key[LC_WAVE], heads = 0, emits = 0;
        for (int lane = 0; lane < LC_WAVE; ++lane) key[lane] = contact_key(cells.data(), g, o, lz, ly, lane, off, with_background, bits);
        for (int lane = 0; lane < LC_WAVE; ++lane) {
          const bool head = run_head(key[lane], lane ? key[lane - 1] : 0, lane);
          if (head) heads |= 1ull << lane;
          if (head && key[lane] != LC_NO_KEY) emits |= 1ull << lane;
        }
        if (!emits) continue;
        const int total = bit_count(emits);
        const long long base = count;                                       // the wave's slots so far (its atomic per tile, advanced row by row)
        count += total;
        if (!out) continue;
        out->resize((size_t)count);
        int seen = 0, covered = 0;
        for (int lane = 0; lane < LC_WAVE; ++lane) {
          if (!((heads >> lane) & 1ull)) continue;
          const int len = run_length(heads, lane);
          if (len < 1 || lane + len > LC_WAVE) return -2;
          for (int j = 0; j < len; ++j) if (key[lane + j] != key[lane]) return -2;    // a run holds one key
          covered += len;
          if (!((emits >> lane) & 1ull)) continue;
          const int slot = run_slot(emits, lane);
          if (slot != seen++) return -2;                                    // the slots of a wave are 0, 1, 2, ... in lane order
          (*out)[(size_t)(base + slot)] = std::make_pair(key[lane], (long long)len);
        }
        if (seen != total || covered != LC_WAVE) return -2;
      }
    }
  }
  return count;
}

// what sd_label_contacts_device computes, with its argument checks; runs: the number of appended runs
static int contacts(const int* lbl, int ndim, int Z, int Y, int X, int connectivity, int with_background, bool reversed,
                    std::vector<long long>& keys, std::vector<long long>& counts, long long* runs) {
  keys.clear(); counts.clear(); *runs = 0;
  if ((ndim != 2 && ndim != 3) || (ndim == 2 && Z != 1)) return -1;
  if (connectivity < 1 || connectivity > ndim) return -1;
  if (Z <= 0 || Y <= 0 || X <= 0) return 0;
  if (!lbl) return -1;
  const Tile g = tile_of(Z, Y, X);
  int mn = INT_MAX, mx = INT_MIN;
  const long long n_runs = pass(lbl, g, reversed, connectivity, with_background, 32, nullptr, &mn, &mx);
  if (n_runs < 0) return (int)n_runs;
  if (mn < 0 || n_runs == 0) return 0;
  const int bits = bits_of(mx);
  if (2 * bits > 62) return -2;
  Runs list;
  if (pass(lbl, g, reversed, connectivity, with_background, bits, &list, &mn, &mx) != n_runs) return -3;     // the two passes agree
  std::sort(list.begin(), list.end());
  for (size_t i = 0; i < list.size(); ++i) {
    const long long k = unpacked_key(list[i].first, bits);
    if (keys.empty() || keys.back() != k) { keys.push_back(k); counts.push_back(0); }
    counts.back() += list[i].second;
  }
  *runs = n_runs;
  return 0;
}

template <typename T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n ? n : 1);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 2) { fprintf(stderr, "usage: %s <records file>\n", argv[0]); return 2; }
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  int records = 0, bad = 0;
  long long combined = 0;                                                   // records whose runs were fewer than their contacts
  for (;;) {
    int head[6];
    long long tail[2];
    if (fread(head, sizeof(int), 6, f) != 6) break;
    if (fread(tail, sizeof(long long), 2, f) != 2) { fprintf(stderr, "truncated record\n"); return 2; }
    const int ndim = head[0], Z = head[1], Y = head[2], X = head[3];
    const size_t n = (size_t)Z * Y * X, m = (size_t)tail[0];
    std::vector<int> lbl;
    std::vector<long long> want_keys, want_counts, keys, counts;
    if (!(read_n(f, lbl, n) && read_n(f, want_keys, m) && read_n(f, want_counts, m))) { fprintf(stderr, "truncated record %d\n", records); return 2; }
    want_keys.resize(m); want_counts.resize(m);
    bool ok = true;
    for (int reversed = 0; reversed < 2; ++reversed) {
      long long runs = 0, sum = 0;
      const int rc = contacts(lbl.data(), ndim, Z, Y, X, head[4], head[5], reversed != 0, keys, counts, &runs);
      for (size_t i = 0; i < counts.size(); ++i) sum += counts[i];
      if (rc != 0 || keys != want_keys || counts != want_counts || runs > sum) {
        ok = false;
        printf("record %d (%d x %d x %d, connectivity %d, background %d, tiles %s): rc %d, %zu rows for %zu\n", records, Z, Y, X, head[4],
               head[5], reversed ? "descending" : "ascending", rc, keys.size(), m);
      }
      if (!reversed && runs < sum) ++combined;
    }
    if (!ok) ++bad;
    ++records;
  }
  fclose(f);
  // the argument checks of the entry point, and the smallest tables
  {
    std::vector<long long> k, c;
    long long runs = 0;
    const int two[2] = {1, 2}, neg[2] = {-1, 2};
    const bool checks = contacts(two, 1, 1, 1, 2, 1, 0, false, k, c, &runs) == -1 && contacts(two, 4, 1, 1, 2, 1, 0, false, k, c, &runs) == -1 &&
                        contacts(two, 2, 2, 1, 1, 1, 0, false, k, c, &runs) == -1 && contacts(two, 2, 1, 1, 2, 0, 0, false, k, c, &runs) == -1 &&
                        contacts(two, 2, 1, 1, 2, 3, 0, false, k, c, &runs) == -1 && contacts(two, 3, 1, 1, 2, 4, 0, false, k, c, &runs) == -1 &&
                        contacts(nullptr, 2, 1, 1, 2, 1, 0, false, k, c, &runs) == -1 &&
                        contacts(nullptr, 2, 1, 0, 2, 1, 0, false, k, c, &runs) == 0 && k.empty() &&
                        contacts(neg, 2, 1, 1, 2, 1, 1, false, k, c, &runs) == 0 && k.empty() &&
                        contacts(two, 2, 1, 1, 2, 1, 0, false, k, c, &runs) == 0 && k.size() == 1 && k[0] == ((1ll << 32) | 2) && c[0] == 1 && runs == 1 &&
                        contacts(two, 3, 1, 1, 2, 3, 0, true, k, c, &runs) == 0 && k.size() == 1 && c[0] == 1;
    if (!checks) { ++bad; printf("argument checks failed\n"); }
  }
  printf("%d records, %d bad, %lld with combined runs\n", records, bad, combined);
  return bad ? 1 : 0;
}
