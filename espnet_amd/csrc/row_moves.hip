// Row moves of the batched transducer searches: what a step kernel decided (parent rows, frames, pool rows) applied to the fp32
// matrices the rest of the step reads - the projected encoder rows, h / c of every prediction-network layer, lin_dec's outputs.
//
//   eamd_gather_rows    up to 16 row gathers dst_j[r, :] = src_j[idx_j[r], :] in one launch; an index is clamped to the source's rows.
//   eamd_scatter_rows   up to 16 masked row scatters dst_j[idx_j[r], :] = src_j[r, :] in one launch; a row whose mask byte is 0 or
//                       whose index is outside the destination is skipped.
// Both take one job per blockIdx.y and move float4s when a job's width and pointers allow it.
#include "common.h"
#include "../../include/espnet_amd.h"

namespace {

struct RowJobs {
  const float* src[16];
  float* dst[16];
  const int* idx[16];
  const unsigned char* mask[16];               // scatter only; the gather leaves it null
  int nrows[16], width[16], other_rows[16], vec[16];   // other_rows: rows of the indexed side (gather: src, scatter: dst)
  int n;
};

__global__ __launch_bounds__(256) void gather_rows_kernel(const RowJobs j) {
  const int job = blockIdx.y;
  if (job >= j.n) return;
  const float* s = j.src[job];
  float* d = j.dst[job];
  const int* idx = j.idx[job];
  const int width = j.width[job], last = j.other_rows[job] - 1;
  if (j.vec[job]) {
    const int wq = width >> 2;
    const long total = (long)j.nrows[job] * wq;
    for (long x = (long)blockIdx.x * 256 + threadIdx.x; x < total; x += (long)gridDim.x * 256) {
      const long r = x / wq;
      const int c = (int)(x - r * wq);
      const long sr = min(max(idx[r], 0), last);
      reinterpret_cast<float4*>(d + r * width)[c] = reinterpret_cast<const float4*>(s + sr * width)[c];
    }
  } else {
    const long total = (long)j.nrows[job] * width;
    for (long x = (long)blockIdx.x * 256 + threadIdx.x; x < total; x += (long)gridDim.x * 256) {
      const long r = x / width;
      const int c = (int)(x - r * width);
      const long sr = min(max(idx[r], 0), last);
      d[r * width + c] = s[sr * width + c];
    }
  }
}

__global__ __launch_bounds__(256) void scatter_rows_kernel(const RowJobs j) {
  const int job = blockIdx.y;
  if (job >= j.n) return;
  const float* s = j.src[job];
  float* d = j.dst[job];
  const int* idx = j.idx[job];
  const unsigned char* mask = j.mask[job];
  const int width = j.width[job], rows = j.other_rows[job];
  const int wq = j.vec[job] ? width >> 2 : width;
  const long total = (long)j.nrows[job] * wq;
  for (long x = (long)blockIdx.x * 256 + threadIdx.x; x < total; x += (long)gridDim.x * 256) {
    const long r = x / wq;
    const int col = (int)(x - r * wq);
    const int dr = idx[r];
    if (dr < 0 || dr >= rows || (mask && !mask[r])) continue;
    if (j.vec[job])
      reinterpret_cast<float4*>(d + (long)dr * width)[col] = reinterpret_cast<const float4*>(s + r * width)[col];
    else
      d[(long)dr * width + col] = s[r * width + col];
  }
}

// validates and packs njobs <= 16 jobs (mask: null for the gather) and sizes the grid's x by the largest job
int pack_row_jobs(RowJobs& j, unsigned& bx, const float* const* src, float* const* dst, const int32_t* const* idx,
                  const uint8_t* const* mask, const int32_t* nrows, const int32_t* width, const int32_t* other_rows, int njobs) {
  long most = 0;
  for (int q = 0; q < 16; ++q) {
    const bool on = q < njobs;
    j.src[q] = on ? src[q] : nullptr;
    j.dst[q] = on ? dst[q] : nullptr;
    j.idx[q] = on ? idx[q] : nullptr;
    j.mask[q] = on && mask ? mask[q] : nullptr;
    j.nrows[q] = j.width[q] = j.other_rows[q] = j.vec[q] = 0;
    if (!on) continue;
    if (!src[q] || !dst[q] || !idx[q] || nrows[q] < 0 || width[q] < 1 || other_rows[q] < 1) return EAMD_EINVAL;
    if ((((uintptr_t)src[q] | (uintptr_t)dst[q] | (uintptr_t)idx[q]) & 3)) return EAMD_EUNSUPPORTED;
    j.nrows[q] = nrows[q];
    j.width[q] = width[q];
    j.other_rows[q] = other_rows[q];
    j.vec[q] = width[q] % 4 == 0 && !(((uintptr_t)src[q] | (uintptr_t)dst[q]) & 15);
    const long work = (long)nrows[q] * (j.vec[q] ? width[q] / 4 : width[q]);
    most = work > most ? work : most;
  }
  j.n = njobs;
  bx = most == 0 ? 1 : (unsigned)((most + 255) / 256 < 64 ? (most + 255) / 256 : 64);
  return EAMD_OK;
}

}  // namespace

extern "C" {

int eamd_gather_rows(const float* const* src, float* const* dst, const int32_t* const* idx, const int32_t* nrows, const int32_t* width,
                     const int32_t* src_rows, int njobs, void* stream) {
  if (!src || !dst || !idx || !nrows || !width || !src_rows || njobs <= 0 || njobs > 16) return EAMD_EINVAL;
  RowJobs j;
  unsigned bx;
  const int rc = pack_row_jobs(j, bx, src, dst, idx, nullptr, nrows, width, src_rows, njobs);
  if (rc != EAMD_OK) return rc;
  hipLaunchKernelGGL(gather_rows_kernel, dim3(bx, njobs), dim3(256), 0, (hipStream_t)stream, j);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

int eamd_scatter_rows(float* const* dst, const float* const* src, const int32_t* const* idx, const uint8_t* const* mask,
                      const int32_t* nrows, const int32_t* width, const int32_t* dst_rows, int njobs, void* stream) {
  if (!dst || !src || !idx || !mask || !nrows || !width || !dst_rows || njobs <= 0 || njobs > 16) return EAMD_EINVAL;
  RowJobs j;
  unsigned bx;
  const int rc = pack_row_jobs(j, bx, src, dst, idx, mask, nrows, width, dst_rows, njobs);
  if (rc != EAMD_OK) return rc;
  hipLaunchKernelGGL(scatter_rows_kernel, dim3(bx, njobs), dim3(256), 0, (hipStream_t)stream, j);
  EAMD_LAUNCH_CHECK();
  return EAMD_OK;
}

}  // extern "C"
