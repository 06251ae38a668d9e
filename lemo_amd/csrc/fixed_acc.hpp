// Order-independent scattered sums: a two-word 64-bit fixed-point accumulator per destination, fed by integer atomics.
// fp32 atomic adds round after every arrival, so their sum depends on the order the waves get there; integer adds do not.
// A destination is two long long words {hi, lo}.  A contribution v is split exactly: hi = rint(v 2^20) units of 2^-20, and the
// remainder v - hi 2^-20 (exactly representable in fp32, below 2^-21 in magnitude, 0 for |v| >= 2^3) goes to lo in units of 2^-60.
//   precision  the only rounding is the remainder's to 2^-60 (8.7e-19): nothing of an fp32 contribution above 2^-36 is lost
//   range      a contribution must be finite and |v| < 2^17; hi then holds sums up to 2^43 -- 2^26 contributions at the cap -- and lo
//              2^24 remainders (2^39 units each).  No realistic sum comes near either
//   not finite / out of range: nothing is added, *flag = 1 (every writer stores the same word); the reader decides what that means
#pragma once
#include "common.hpp"

namespace lemo {

#define LEMO_FIX_WORDS 2
#define LEMO_FIX_LIMIT 131072.0f                  // 2^17

// acc: the buffer's base, i: the destination's index
__device__ __forceinline__ void fix_add(long long* acc, size_t i, float v, int* flag) {
  if (v == 0.f) return;
  if (!(fabsf(v) < LEMO_FIX_LIMIT)) { *flag = 1; return; }
  const float hi = rintf(v * 1048576.0f);                                    // 2^20; |hi| < 2^37, an integer
  const float lo = v - hi * (1.0f / 1048576.0f);                             // exact
  unsigned long long* w = reinterpret_cast<unsigned long long*>(acc + LEMO_FIX_WORDS * i);
  if (hi != 0.f) atomicAdd(w, static_cast<unsigned long long>(static_cast<long long>(hi)));
  if (lo != 0.f) atomicAdd(w + 1, static_cast<unsigned long long>(llrintf(lo * 1152921504606846976.0f)));      // 2^60
}
__device__ __forceinline__ float fix_value(const long long* acc, size_t i) {
  const long long hi = acc[LEMO_FIX_WORDS * i], lo = acc[LEMO_FIX_WORDS * i + 1];
  return (float)((double)hi * (1.0 / 1048576.0) + (double)lo * (1.0 / 1152921504606846976.0));
}

}  // namespace lemo
