// sample_rng.h -- the counter-based uniform of cv_sample_batch (include/cviterbi.h, "posterior
// path sampling"): u(seed, S, r, t) in [0, 1), a pure function of the global sequence index S,
// the draw r and the position t, so a draw depends on nothing around it.  One definition for the
// kernels (sample.hip) and the host (a unit check can call it); cviterbi/sample.py mirrors it.
#ifndef CV_KERNELS_SAMPLE_RNG_H
#define CV_KERNELS_SAMPLE_RNG_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define CVS_HD __host__ __device__ __forceinline__
#else
#define CVS_HD inline
#endif

namespace cvs {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kStepMul = 0xD1B54A32D192ED03ull;

CVS_HD uint64_t mix(uint64_t z) {  // the splitmix64 finaliser
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}

// the key of (seed, sequence S, draw r): three of the four rounds, once per walk
CVS_HD uint64_t draw_key(uint64_t seed, uint64_t S, uint64_t r) {
  uint64_t k = mix(seed + kGolden);
  k = mix(k ^ S);
  return mix(k + kGolden * (r + 1));
}

// the uniform of position t under a key: 53 bits, exact in f64
CVS_HD double key_uniform(uint64_t key, uint64_t t) {
  const uint64_t z = mix(key ^ (t * kStepMul));
  return (double)(z >> 11) * 0x1.0p-53;
}

CVS_HD double uniform(uint64_t seed, uint64_t S, uint64_t r, uint64_t t) { return key_uniform(draw_key(seed, S, r), t); }

}  // namespace cvs

#endif  // CV_KERNELS_SAMPLE_RNG_H
