// Host harness of stardist_amd/csrc/select_rank.h: the digit-by-digit selection of csrc/normalize.hip on host arrays, with the header's
// own keys, digit plan, find_bin and interpolation.  The histogram loop below stands in for the device's histogram kernels; everything
// else is the code the device runs.  Built by tests/test_cpu_normalize.py (g++ -ffp-contract=off, as the library is).
#include <stdint.h>
#include <vector>
#include "../../stardist_amd/csrc/select_rank.h"

using namespace selrank;

namespace {

template <typename T>
void select_keys(const T* x, long long n, int dtype, const long long* ranks, int nr, uint32_t* keys) {
  std::vector<uint32_t> prefix(nr, 0u);
  std::vector<unsigned long long> rank(nr);
  for (int s = 0; s < nr; ++s) rank[s] = (unsigned long long)ranks[s];
  for (int pass = 0; pass < n_passes(dtype); ++pass) {
    const int nb = 1 << digit_bits(dtype, pass);
    // one histogram per distinct prefix (the device fills the first slot that carries it); here: one per slot, filled in one sweep
    std::vector<int> owner(nr);
    for (int s = 0; s < nr; ++s) { owner[s] = s; for (int j = 0; j < s; ++j) if (prefix[j] == prefix[s]) { owner[s] = j; break; } }
    std::vector<std::vector<unsigned long long>> hist(nr);
    for (int s = 0; s < nr; ++s) if (owner[s] == s) hist[s].assign(nb, 0ull);
    for (long long i = 0; i < n; ++i) {
      const uint32_t k = key_of(x[i]);
      const uint32_t p = prefix_of(k, dtype, pass);
      for (int s = 0; s < nr; ++s) if (owner[s] == s && (pass == 0 || prefix[s] == p)) { ++hist[s][digit_of(k, dtype, pass)]; break; }
    }
    for (int s = 0; s < nr; ++s) {
      const int b = find_bin(hist[owner[s]].data(), nb, &rank[s]);
      prefix[s] = (pass == 0 ? 0u : prefix[s] << digit_bits(dtype, pass)) | (uint32_t)b;
    }
  }
  for (int s = 0; s < nr; ++s) keys[s] = prefix[s];
}

void keys_for(const void* x, int dtype, long long n, const long long* ranks, int nr, uint32_t* keys) {
  if (dtype == DT_U8) select_keys((const uint8_t*)x, n, dtype, ranks, nr, keys);
  else if (dtype == DT_U16) select_keys((const uint16_t*)x, n, dtype, ranks, nr, keys);
  else select_keys((const float*)x, n, dtype, ranks, nr, keys);
}

}  // namespace

extern "C" {

// values[s] = the element of rank ranks[s] (0-based) of x, as a double
void sr_select(const void* x, int dtype, long long n, const long long* ranks, int nr, double* values) {
  std::vector<uint32_t> keys(nr);
  keys_for(x, dtype, n, ranks, nr, keys.data());
  for (int s = 0; s < nr; ++s) values[s] = dtype == DT_F32 ? (double)f32_of_key(keys[s]) : (double)keys[s];
}

// out[j] = float32(np.percentile(x, q[j])) the way sd_percentiles_device builds it; ranks_out (2 per q) receives the ranks it asked for
void sr_percentile(const void* x, int dtype, long long n, const double* q, int nq, int interp_f32, float* out, long long* ranks_out) {
  const bool f32 = dtype == DT_F32 && interp_f32;
  std::vector<long long> ranks(2 * nq);
  std::vector<Lerp> plan(nq);
  for (int j = 0; j < nq; ++j) { plan[j] = lerp_plan(n, q[j], f32); ranks[2 * j] = plan[j].lo; ranks[2 * j + 1] = plan[j].hi; }
  std::vector<uint32_t> keys(2 * nq);
  keys_for(x, dtype, n, ranks.data(), 2 * nq, keys.data());
  for (int j = 0; j < nq; ++j) {
    const uint32_t ka = keys[2 * j], kb = keys[2 * j + 1];
    if (dtype == DT_F32) {
      const float a = f32_of_key(ka), b = f32_of_key(kb);
      out[j] = f32 ? lerp_f32(a, b, (float)plan[j].t) : (float)lerp_f64((double)a, (double)b, plan[j].t);
    } else {
      out[j] = (float)lerp_f64((double)ka, (double)kb, plan[j].t);
    }
    ranks_out[2 * j] = ranks[2 * j]; ranks_out[2 * j + 1] = ranks[2 * j + 1];
  }
}

}  // extern "C"
