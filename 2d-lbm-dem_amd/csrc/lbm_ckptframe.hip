// lbm_ckptframe.hip -- one checkpoint as the file holds it: the device-resident sections lbmdem_checkpoint_save dumps one by
// one -- r, kin[kcur] (9n), fhf (3n), gp, V.offsets (n + 1 ints), V.nbr (offsets[n] ints, read here), V.wallflags (n bytes),
// obst[ocur], the nine planes of f[fcur], and behind them the optional state a handle was told to save
// (lbmdem_set_checkpoint_contents): the tracers' xy, the scalar's g[cur] and was, the window's cnt and S -- gathered into a
// slot's staging by ONE launch on the handle's stream, with every section's digest added up in the same pass (lbmdem_checkpoint_save_async; layout: CkptFrameJob, lbmdem_internal.h).
// Double-precision library only: the float build has no checkpoints.
#include "lbmdem_internal.h"

#ifndef LBMDEM_SINGLE_PRECISION
namespace {

typedef unsigned long long u64;
constexpr int CKPT_BLOCK = 256;
constexpr int CKPT_MAX_BLOCKS = 2048;   // a memory-bound copy: the rest is a grid-stride loop

// Bytes [16 c, 16 c + 16) of a section of `bytes` bytes as its little-endian words 2 c and 2 c + 1. Nothing beyond the section's
// end is read: the last chunk of a section that is no multiple of 16 bytes long (wallflags: n bytes; nbr: an odd number of
// ints as often as not) is read byte by byte and zero-padded. A whole chunk is one 16-byte load where the section starts on
// a 16-byte boundary -- obst, f and the lists do; the grains' arrays are carved from one allocation in pieces of n doubles and
// do only when n is even -- else in the widest pieces its start allows.
__device__ __forceinline__ void ckpt_load16(const unsigned char* __restrict__ src, size_t bytes, size_t c, int align, u64& w0,
                                            u64& w1) {
  w0 = 0; w1 = 0;
  if (!src) return;
  const size_t b0 = 16 * c;
  const unsigned char* p = src + b0;
  if (b0 + 16 <= bytes) {
    if (align == 16) {
      const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(p);
      w0 = v.x; w1 = v.y;
    } else if (align == 8) {
      w0 = reinterpret_cast<const u64*>(p)[0]; w1 = reinterpret_cast<const u64*>(p)[1];
    } else if (align == 4) {
      const unsigned* q = reinterpret_cast<const unsigned*>(p);
      w0 = q[0] | ((u64)q[1] << 32); w1 = q[2] | ((u64)q[3] << 32);
    } else {
      for (int k = 0; k < 8; ++k) { w0 |= (u64)p[k] << (8 * k); w1 |= (u64)p[8 + k] << (8 * k); }
    }
  } else {
    const int left = (int)(bytes - b0);   // 1 .. 15
    for (int k = 0; k < left; ++k) {
      if (k < 8) w0 |= (u64)p[k] << (8 * k);
      else w1 |= (u64)p[k] << (8 * (k - 8));
    }
  }
}

// One section: copied in 16-byte chunks, grid-stride, every lane adding the two words of its chunks to its own S1 and S2 (a
// word is counted by exactly one lane); then the wavefront's sums by shuffles, the workgroup's through 64 bytes of LDS, and ONE
// integer atomicAdd per workgroup and sum -- integer sums are associative, any order gives the same bits.
template <int S>
__device__ __forceinline__ void ckpt_section(const CkptFrameJob& J, size_t bytes, u64 (*part)[2]) {
  const size_t chunks = (bytes + 15) / 16;
  if ((size_t)blockIdx.x * CKPT_BLOCK >= chunks) return;   // (the same for the whole workgroup)
  const unsigned char* src = static_cast<const unsigned char*>(J.src[S]);
  const size_t a = reinterpret_cast<size_t>(src);
  const int align = (a & 15) == 0 ? 16 : ((a & 7) == 0 ? 8 : ((a & 3) == 0 ? 4 : 1));
  ulonglong2* dst = reinterpret_cast<ulonglong2*>(J.staging + J.at[S]);
  const size_t stride = (size_t)gridDim.x * CKPT_BLOCK;
  u64 s1 = 0, s2 = 0;
  for (size_t c = (size_t)blockIdx.x * CKPT_BLOCK + threadIdx.x; c < chunks; c += stride) {
    u64 w0, w1;
    ckpt_load16(src, bytes, c, align, w0, w1);
    ulonglong2 v;
    v.x = w0; v.y = w1;
    dst[c] = v;
    s1 += w0 + w1;
    s2 += (2 * (u64)c + 1) * w0 + (2 * (u64)c + 2) * w1;
  }
  for (int d = 32; d > 0; d >>= 1) {
    s1 += __shfl_xor(s1, d);
    s2 += __shfl_xor(s2, d);
  }
  if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = s1; part[threadIdx.x >> 6][1] = s2; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < CKPT_BLOCK / 64; ++k) { s1 += part[k][0]; s2 += part[k][1]; }
    u64* words = reinterpret_cast<u64*>(J.staging);
    atomicAdd(words + 4 + 2 * S, s1);
    atomicAdd(words + 5 + 2 * S, s2);
  }
  __syncthreads();   // (part is the next section's too)
}

__global__ __launch_bounds__(CKPT_BLOCK) void k_ckpt_frame(const CkptFrameJob J) {
  LBMDEM_GATE(J.gate);
  __shared__ u64 part[CKPT_BLOCK / 64][2];
  // the pair list's length is on the device only: every lane reads the one word
  const int nn = J.nnbr ? *J.nnbr : 0;
  size_t nbr_bytes = nn > 0 ? 4 * (size_t)nn : 0;
  if (nbr_bytes > J.bytes[CKPT_NBR]) nbr_bytes = J.bytes[CKPT_NBR];   // (never beyond the list's capacity)
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    u64* words = reinterpret_cast<u64*>(J.staging);
    words[0] = nbr_bytes / 4;
    for (int k = 0; k < 3; ++k) words[1 + k] = (u64)__double_as_longlong(J.carry[k]);
  }
  ckpt_section<CKPT_R>(J, J.bytes[CKPT_R], part);
  ckpt_section<CKPT_KIN>(J, J.bytes[CKPT_KIN], part);
  ckpt_section<CKPT_FHF>(J, J.bytes[CKPT_FHF], part);
  ckpt_section<CKPT_GP>(J, J.bytes[CKPT_GP], part);
  ckpt_section<CKPT_OFFSETS>(J, J.bytes[CKPT_OFFSETS], part);
  ckpt_section<CKPT_NBR>(J, nbr_bytes, part);
  ckpt_section<CKPT_WALLFLAGS>(J, J.bytes[CKPT_WALLFLAGS], part);
  ckpt_section<CKPT_OBST>(J, J.bytes[CKPT_OBST], part);
  ckpt_section<CKPT_F>(J, J.bytes[CKPT_F], part);
  // the optional state: length 0 (nothing read, nothing written, no atomic) where the file does not carry it
  ckpt_section<CKPT_TRACERS>(J, J.bytes[CKPT_TRACERS], part);
  ckpt_section<CKPT_SCALAR_G>(J, J.bytes[CKPT_SCALAR_G], part);
  ckpt_section<CKPT_SCALAR_WAS>(J, J.bytes[CKPT_SCALAR_WAS], part);
  ckpt_section<CKPT_MEAN_CNT>(J, J.bytes[CKPT_MEAN_CNT], part);
  ckpt_section<CKPT_MEAN_S>(J, J.bytes[CKPT_MEAN_S], part);
}

}  // namespace

void launch_ckpt_frame(const CkptFrameJob& J, hipStream_t st) {
  size_t most = 1;
  for (int s = 0; s < CKPT_ALL_SECTIONS; ++s) {   // all fourteen: the scalar's or the window's planes may be the longest
    const size_t chunks = (J.bytes[s] + 15) / 16;
    if (chunks > most) most = chunks;
  }
  size_t blocks = (most + CKPT_BLOCK - 1) / CKPT_BLOCK;
  if (blocks > CKPT_MAX_BLOCKS) blocks = CKPT_MAX_BLOCKS;
  hipLaunchKernelGGL(k_ckpt_frame, dim3((unsigned)blocks), dim3(CKPT_BLOCK), 0, st, J);
}
#endif
