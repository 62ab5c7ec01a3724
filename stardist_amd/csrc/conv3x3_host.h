// conv3x3_host.h -- host side shared by the three forms of the 3x3 / 3x3x3 convolution (conv3x3.hip: exact f32; conv3x3_bf16.hip:
// bf16x6; conv3x3_f16.hip: f16x3): the checks every form makes on its arguments, the launch descriptor (conv3x3_device.h Params) and the
// grid of a persistent launch.  Everything up to the grid runs before the first HIP call (tests/test_cpu_conv_launch_args.py).
#pragma once
#include "common.h"
#include "conv3x3_device.h"

namespace sdconvhost {

using namespace sdconvdev;

struct Source {
  const float* p;      // channels-last; src[1].p == nullptr: the layer has one source
  int c, stride, up;   // channels read, floats per pixel, up-sampling mask (bit 0 x, bit 1 y, bit 2 z)
};
struct Args {
  Source src[2];
  int D, H, W, kz;
  const float* wp;     // packed weights, followed by 16 bytes of zeros
  const float* bias;
  const float* res;    // optional residual and its floats per pixel
  int res_stride;
  int c_out, act;
  float* out;
  int* flag = nullptr;      // f16x3: range flag
  bool no_out = false;      // f16x3: the fused head without the feature store (out == nullptr)
};

// The first check of every form.  n_packed: the form's packed weight floats for these channel counts and kz, < 0: unsupported
inline int check_args(const char* form, const Args& a, long long n_packed) {
  const Source &s0 = a.src[0], &s1 = a.src[1];
  if (!s0.p || !a.wp || (!a.out && !a.no_out) || (a.act != 0 && a.act != 1) || n_packed < 0 || (a.kz == 1 && a.D != 1) ||
      (((uintptr_t)s0.p | (uintptr_t)s1.p | (uintptr_t)a.wp | (uintptr_t)a.out | (uintptr_t)a.bias) & 15) || ((uintptr_t)a.flag & 3)) {
    sd::set_error("%s: unsupported channel counts (%d + %d -> %d), kz, act or misaligned pointers", form, s0.c, s1.p ? s1.c : 0, a.c_out);
    return -1;
  }
  return 0;
}

// Arguments -> launch descriptor: every check the forms share, in the order arguments, up masks, sources, residual, tile count (the
// first one that fails sets the message, prefixed with the form's name), and all of P; the fused head is left empty (dotw, dotp).
// 0, or -1 + error set.  The caller has returned already when D, H or W <= 0 (nothing to do).
inline int prepare(const char* form, const Args& a, long long n_packed, Params& P) {
  if (check_args(form, a, n_packed)) return -1;
  const Source &s0 = a.src[0], &s1 = a.src[1];
  const bool two = s1.p != nullptr;
  for (const int up : {s0.up, two ? s1.up : 0})
    if (up < 0 || up > 7 || ((up & 1) && (a.W & 1)) || ((up & 2) && (a.H & 1)) || ((up & 4) && (a.D & 1))) {
      sd::set_error("%s: up is a bit mask (1: x, 2: y, 4: z); an up-sampled axis needs an even output size", form);
      return -1;
    }
  if ((s0.c % 32) || (two && (s1.c % 32)) || s0.stride < s0.c || (s0.stride & 3) || (two && (s1.stride < s1.c || (s1.stride & 3)))) {
    sd::set_error("%s: sources must hold multiples of 32 channels, strides multiples of 4 floats", form);
    return -1;
  }
  if (a.res && (a.res_stride < a.c_out || (a.res_stride & 3) || ((uintptr_t)a.res & 15))) {
    sd::set_error("%s: the residual needs 16-byte alignment and a stride >= c_out", form);
    return -1;
  }
  // 64-bit until the count is known to fit: 2^20 x 2^20 pixels are 2^32 tiles
  const long long tiles_x = ((long long)a.W + TW - 1) / TW, tiles_plane = tiles_x * (((long long)a.H + TH - 1) / TH);      // < 2^54
  if (tiles_plane > 0x7fffffffLL || tiles_plane * a.D > 0x7fffffffLL) {
    sd::set_error("%s: too many tiles", form);
    return -1;
  }
  int nc = 0;
  P.kind[0] = make_src(s0.p, s0.stride, s0.up, a.H, a.W);
  P.kind[1] = two ? make_src(s1.p, s1.stride, s1.up, a.H, a.W) : P.kind[0];
  for (int k = 0; k < MAX_CHUNKS; ++k) { P.chunk_kind[k] = 0; P.chunk_choff[k] = 0; }
  for (int k = 0; k < s0.c / 32; ++k) { P.chunk_kind[nc] = 0; P.chunk_choff[nc++] = k * 32; }
  if (two) for (int k = 0; k < s1.c / 32; ++k) { P.chunk_kind[nc] = 1; P.chunk_choff[nc++] = k * 32; }
  P.D = a.D; P.H = a.H; P.W = a.W; P.kz = a.kz; P.n_units = nc * a.kz; P.n_chunks0 = s0.c / 32;
  P.zero = a.wp + (n_packed - 4);
  P.res = a.res; P.res_stride = a.res_stride;
  P.wp = a.wp; P.bias = a.bias; P.out = a.out; P.c_out = a.c_out; P.act = a.act;
  P.flag = a.flag; P.dotw = nullptr; P.dotp = nullptr;
  P.tiles_x = (int)tiles_x; P.tiles_plane = (int)tiles_plane; P.n_tiles = (int)(tiles_plane * a.D);
  P.groups = a.c_out / 32;
  return 0;
}

// Grid of a persistent launch: per_cu workgroups per CU, a whole number per output-channel group (wg_slot), at least one and at most
// n_tiles per group.  `kernels`: every instance the caller may launch with `lds` bytes of dynamic LDS; `attr_done`: the caller's
// record, zero-initialised, that they have been allowed that much on a device (sd::allow_dynamic_lds).  0, or -1 + error set.
template <int N>
inline int persistent_grid(const void* const (&kernels)[N], bool (&attr_done)[sd::kMaxDevices], size_t lds, const Params& P, int per_cu, unsigned& blocks) {
  if (sd::allow_dynamic_lds(kernels, N, (int)lds, attr_done)) return -1;
  const int cus = sd::cu_count();
  if (cus <= 0) return -1;
  long long n = (long long)(per_cu * cus / P.groups) * P.groups;
  if (n < P.groups) n = P.groups;
  const long long want = (long long)P.n_tiles * P.groups;
  if (n > want) n = want;
  blocks = (unsigned)n;
  return 0;
}

}  // namespace sdconvhost
