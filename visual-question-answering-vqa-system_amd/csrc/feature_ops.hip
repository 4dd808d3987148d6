// Row gather for cached image features (VQAModel.encode_features / ImageFeatures.select):
//   gather_rows_kernel : dst[i] = src[index[i]] over rows of row_bytes bytes (a multiple of 16), any element type
//
// A row is a 7 x 7 x 512 bf16 feature block (50 176 B) at the default shape, 147 456 B at the 384 px stress shape: pure HBM traffic,
// one read and one write of n * row_bytes.  One workgroup of 256 lanes moves one 16 KB chunk of one row: every lane issues its four
// 16-byte loads (lane-contiguous, 4 KB per wave instruction) before the first store, so four loads per lane are in flight.  The last
// chunk of a row is partial when row_bytes is no multiple of 16 KB (49 x 512 bf16: 3 full chunks + 1 KB); cutting a row into equal
// chunks instead is untried.
#include "common.h"

namespace {

constexpr int GATHER_THREADS = 256;
constexpr int GATHER_VECS = 4;                                   // 16-byte vectors per lane
constexpr unsigned GATHER_CHUNK = GATHER_THREADS * GATHER_VECS;  // vectors per workgroup (16 KB)

__global__ __launch_bounds__(GATHER_THREADS) void gather_rows_kernel(const u32x4* __restrict__ src, const int* __restrict__ index,
                                                                     u32x4* __restrict__ dst, unsigned vecs, unsigned chunks, int n_src) {
  const unsigned row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
  const int s = index[row];
  if ((unsigned)s >= (unsigned)n_src) return;                    // (the caller checks the range; a bad entry never reads out of bounds)
  const u32x4* sp = src + (size_t)s * vecs;
  u32x4* dp = dst + (size_t)row * vecs;
  const unsigned v0 = chunk * GATHER_CHUNK + threadIdx.x;
  u32x4 r[GATHER_VECS];
#pragma unroll
  for (int j = 0; j < GATHER_VECS; ++j) {
    const unsigned v = v0 + j * GATHER_THREADS;
    if (v < vecs) r[j] = sp[v];
  }
#pragma unroll
  for (int j = 0; j < GATHER_VECS; ++j) {
    const unsigned v = v0 + j * GATHER_THREADS;
    if (v < vecs) dp[v] = r[j];
  }
}

}  // namespace

extern "C" {

int vqa_gather_rows(const void* src, const int* index, void* dst, int n, long long row_bytes, int n_src, hipStream_t st) {
  if (n < 0 || n_src < 0 || row_bytes <= 0 || (row_bytes % 16) || row_bytes / 16 > 0x7fffffffll) return VQA_EARG;
  if (n == 0) return VQA_OK;
  if (!src || !index || !dst || n_src == 0 || ((uintptr_t)src % 16) || ((uintptr_t)dst % 16)) return VQA_EARG;
  const unsigned vecs = (unsigned)(row_bytes / 16);
  const unsigned chunks = (vecs + GATHER_CHUNK - 1) / GATHER_CHUNK;
  if ((long long)n * chunks >= (1ll << 24)) return VQA_EARG;      // gridDim.x * blockDim.x stays below 2^32 (83 k default rows: 2^18.3 chunks)
  hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)n * chunks), dim3(GATHER_THREADS), 0, st, (const u32x4*)src, index, (u32x4*)dst,
                     vecs, chunks, n_src);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

}  // extern "C"
