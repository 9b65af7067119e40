// Shared by the batched transducer search kernels (rnnt_alsd.hip, rnnt_tsd.hip, rnnt_nsc.hip).
#pragma once

// numpy.logaddexp on doubles (npy_logaddexp)
__device__ __forceinline__ double al_logaddexp(double a, double b) {
  if (a == b) return a + 0.693147180559945309417232121458176568;
  const double d = a - b;
  if (d > 0) return a + log1p(exp(-d));
  if (d <= 0) return b + log1p(exp(d));
  return d;                                    // NaN
}
