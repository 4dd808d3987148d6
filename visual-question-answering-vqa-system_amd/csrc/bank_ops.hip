// Batch draw from a resident uint8 image bank (dropin/data/image_bank.py ImageBank.batch):
//   bank_batch_kernel : out[b][y][x][c] = bank[rows[b]][cy_b + y][cx_b + (flip_b ? O-1-x : x)][c]   -- bytes are moved, never computed on
//
// A sample is O rows of O*3 bytes cut out of an S x S x 3 image: pure HBM traffic, one read and one write of B * O*O*3 bytes.  The unit
// of work is a GROUP of four pixels (12 bytes = three dwords of the output row: O % 4 == 0, so a row is whole groups and every group
// starts on a dword of `out`).  Lanes take consecutive groups of the sample, so a wave writes 768 contiguous bytes and reads the same
// span of a bank row (two spans where it crosses a row end).
//
// The source of a group starts at byte (cx + 4g) * 3 of its bank row: 12g is a multiple of 4 and so are the row pitch S*3 and the
// image size, so the misalignment r = (cx * 3) % 4 is ONE value per sample.  A lane loads the aligned dwords that hold its 12 bytes --
// three when r == 0, four otherwise, every one of them holding a byte it needs, so nothing outside the bank is read (the bank starts
// and ends on a dword) -- and v_alignbyte shifts them down by r bytes.  A flipped sample reads the mirrored group (same r: the
// mirrored start is a multiple of four pixels too) and reverses its four pixels in registers.
// A workgroup of 256 lanes moves a chunk of 1024 groups (12 KB) of one sample; every lane issues the loads of its four groups before
// its first store.  The grid is (chunks, samples), both clamped and looped over, so one launch serves any B.
#include "common.h"

namespace {

constexpr int BANK_THREADS = 256;
constexpr int BANK_GROUPS = 4;                                     // four-pixel groups per lane
constexpr unsigned BANK_CHUNK = BANK_THREADS * BANK_GROUPS;        // groups per workgroup pass (12 KB of output)
constexpr unsigned BANK_GRID_X = 1024, BANK_GRID_Y = 4096;         // grid clamps: at most 2^30 threads per launch
constexpr int BANK_MAX_SIDE = 32768;                               // S*S*3 stays below 2^32: offsets inside one image are 32-bit

// byte i (0 ... 11) of the 12 bytes held by w0, w1, w2
__device__ __forceinline__ uint32_t bank_byte(uint32_t w0, uint32_t w1, uint32_t w2, int i) {
  const uint32_t w = i < 4 ? w0 : (i < 8 ? w1 : w2);
  return (w >> (8 * (i & 3))) & 0xffu;
}
// the dword made of bytes a, b, c, d (lowest first) of those 12
__device__ __forceinline__ uint32_t bank_pack(uint32_t w0, uint32_t w1, uint32_t w2, int a, int b, int c, int d) {
  return bank_byte(w0, w1, w2, a) | (bank_byte(w0, w1, w2, b) << 8) | (bank_byte(w0, w1, w2, c) << 16) | (bank_byte(w0, w1, w2, d) << 24);
}

__global__ __launch_bounds__(BANK_THREADS) void bank_batch_kernel(const uint8_t* __restrict__ bank, long long n_rows, unsigned S,
                                                                  const int* __restrict__ rows, const int* __restrict__ crop_yx,
                                                                  const uint8_t* __restrict__ flip, uint8_t* __restrict__ out, int B,
                                                                  unsigned O, int* __restrict__ err) {
  const unsigned G = O >> 2, groups = O * G, chunks = (groups + BANK_CHUNK - 1) / BANK_CHUNK;
  const unsigned pitch = S * 3u >> 2;                              // dwords per bank row (S % 4 == 0)
  const int slack = (int)(S - O);
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int row = rows[b];
    const int cy = crop_yx ? crop_yx[2 * b] : 0, cx = crop_yx ? crop_yx[2 * b + 1] : 0;
    if (row < 0 || (long long)row >= n_rows || cy < 0 || cx < 0 || cy > slack || cx > slack) {     // reads nothing, writes nothing
      if (err && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(err, 1);
      continue;
    }
    const bool fl = flip && flip[b];
    const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(bank + (size_t)row * ((size_t)S * S * 3u));
    uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(out + (size_t)b * ((size_t)O * O * 3u));
    const unsigned first = ((unsigned)cy * S + (unsigned)cx) * 3u;  // byte of the window's first pixel inside the image
    const unsigned d0 = first >> 2, r = first & 3u;                 // its dword, and the misalignment every group of the sample shares
    for (unsigned chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
      const unsigned t0 = chunk * BANK_CHUNK + threadIdx.x;
      uint32_t w[BANK_GROUPS][4];
#pragma unroll
      for (int j = 0; j < BANK_GROUPS; ++j) {
        const unsigned t = t0 + j * BANK_THREADS;
        if (t < groups) {
          const unsigned y = t / G, g = t - y * G;
          const uint32_t* p = src + (d0 + y * pitch + (fl ? G - 1 - g : g) * 3u);
          w[j][0] = p[0]; w[j][1] = p[1]; w[j][2] = p[2];
          w[j][3] = r ? p[3] : 0u;                                  // (r == 0: the fourth dword holds nothing of this group)
        }
      }
#pragma unroll
      for (int j = 0; j < BANK_GROUPS; ++j) {
        const unsigned t = t0 + j * BANK_THREADS;
        if (t < groups) {
          const uint32_t a0 = __builtin_amdgcn_alignbyte(w[j][1], w[j][0], r);
          const uint32_t a1 = __builtin_amdgcn_alignbyte(w[j][2], w[j][1], r);
          const uint32_t a2 = __builtin_amdgcn_alignbyte(w[j][3], w[j][2], r);
          uint32_t* q = dst + (size_t)t * 3u;
          if (fl) {                                                 // pixels 3, 2, 1, 0 of the mirrored group, channels in order
            q[0] = bank_pack(a0, a1, a2, 9, 10, 11, 6);
            q[1] = bank_pack(a0, a1, a2, 7, 8, 3, 4);
            q[2] = bank_pack(a0, a1, a2, 5, 0, 1, 2);
          } else {
            q[0] = a0; q[1] = a1; q[2] = a2;
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" {

int vqa_bank_batch(const uint8_t* bank, long long n_rows, int S, const int* rows, const int* crop_yx, const uint8_t* flip,
                   uint8_t* out, int B, int O, int* err, hipStream_t st) {
  if (n_rows < 1 || B < 0 || S < 4 || O < 4 || (S % 4) || (O % 4) || O > S || S > BANK_MAX_SIDE) return VQA_EARG;
  if (B == 0) return VQA_OK;
  if (!bank || !rows || !out || ((uintptr_t)bank % 16) || ((uintptr_t)out % 16)) return VQA_EARG;
  const unsigned groups = (unsigned)O * ((unsigned)O >> 2), chunks = (groups + BANK_CHUNK - 1) / BANK_CHUNK;
  const dim3 grid(chunks < BANK_GRID_X ? chunks : BANK_GRID_X, (unsigned)B < BANK_GRID_Y ? (unsigned)B : BANK_GRID_Y);
  hipLaunchKernelGGL(bank_batch_kernel, grid, dim3(BANK_THREADS), 0, st, bank, n_rows, (unsigned)S, rows, crop_yx, flip, out, B,
                     (unsigned)O, err);
  VQA_LAUNCH_CHECK(); return VQA_OK;
}

}  // extern "C"
