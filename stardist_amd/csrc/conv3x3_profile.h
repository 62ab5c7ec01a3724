// conv3x3_profile.h -- phase timing of the split-bf16 and split-fp16 kernels for tools/conv_phase_profile.hip and
// tools/conv_f16_phase_profile.hip, which compile the kernel source with SD_CONV_PROFILE (never defined in the library build): s_memtime
// stamps at the phase boundaries, summed over the workgroups' first lanes.  The including file defines SD_CONV_PROF_PHASES first.
#pragma once

#ifdef SD_CONV_PROFILE
__device__ unsigned long long g_conv_prof[SD_CONV_PROF_PHASES + 2];   // [0] total, [1 .. PHASES] phases, [PHASES + 1] units
#define PROF_DECL unsigned long long pf_t = __builtin_amdgcn_s_memtime(), pf_acc[SD_CONV_PROF_PHASES] = {}; const unsigned long long pf_t0 = pf_t; unsigned long long pf_units = 0
#define PROF(k) do { const unsigned long long n_ = __builtin_amdgcn_s_memtime(); pf_acc[k] += n_ - pf_t; pf_t = n_; } while (0)
#define PROF_UNIT() (++pf_units)
#define PROF_END() do { if (threadIdx.x == 0) { atomicAdd(&g_conv_prof[0], __builtin_amdgcn_s_memtime() - pf_t0); \
  for (int k_ = 0; k_ < SD_CONV_PROF_PHASES; ++k_) atomicAdd(&g_conv_prof[1 + k_], pf_acc[k_]); atomicAdd(&g_conv_prof[SD_CONV_PROF_PHASES + 1], pf_units); } } while (0)
#else
#define PROF_DECL
#define PROF(k)
#define PROF_UNIT()
#define PROF_END()
#endif
