// bf16 matrix-core vocabulary of the kernel files (internal, device-only): vector types, fp32 <-> bf16 hi/lo conversion, the
// hardware-transposing LDS read, LDS-DMA, and the swizzled images of the LDS-DMA ring with their fragment reader.
// A helper lives in a .hip file while it has one user; the second user moves it here (tests/test_csrc_shared_host.py).
#pragma once
#include "crw_common.h"

namespace crw {

typedef __bf16 bf8 __attribute__((ext_vector_type(8)));  // one MFMA operand fragment: 8 bf16 per lane
typedef short s4v __attribute__((ext_vector_type(4)));   // what one transposed 64-bit LDS read returns
typedef short s8v __attribute__((ext_vector_type(8)));
typedef uint32_t u4v __attribute__((ext_vector_type(4)));  // 16 bytes in flight between global memory and LDS
typedef __attribute__((address_space(3))) char *lds_cp;

// fp32 -> bf16 (round to nearest even) and back; an fp32 value is carried as hi = f2bf(v) plus lo = bf_lo(v, hi), the bf16
// of what hi left over: hi + lo equals v to ~2^-17 relative, and Ah*Bh + Ah*Bl + Al*Bh is an fp32-grade product.
__device__ inline uint16_t f2bf(float x) { return __builtin_bit_cast(uint16_t, (__bf16)x); }
__device__ inline float bf2f(uint16_t h) { return __builtin_bit_cast(float, (uint32_t)h << 16); }
__device__ inline uint16_t bf_lo(float v, uint16_t h) { return f2bf(v - bf2f(h)); }

__device__ inline f32x4 mfma(bf8 a, bf8 b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0); }

// the 32-bit LDS byte address of a pointer into shared memory (what the DS instructions below take)
__device__ inline uint32_t lds_addr_of(const char *p) { return (uint32_t)(uintptr_t)(lds_cp)p; }

// LDS-DMA: every lane moves 16 bytes from its own global address to lds_wave_base + 16 * lane (1 KiB per wave-instruction),
// so an LDS image is lane-linear and any bank swizzle has to be applied to the per-lane SOURCE address.
__device__ inline void glds16(const uint16_t *g, char *lds_wave_base) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)g,
                                   (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, 0);
}

// The transposed LDS read goes through inline asm: given the builtin, hipcc (ROCm 7.2) drains every in-flight LDS-DMA
// (s_waitcnt vmcnt(0)) in front of it, which serialises the ring.  The same holds for the register staging and the LDS stores
// of kernels that keep such a ring (gemm_bf16.hip).  Inline-asm reads are invisible to the compiler's lgkmcnt bookkeeping: the
// caller issues lds_reads_landed(), or a counted wait of its own, before the MFMAs that consume the result.
// OFF is an instruction immediate (0 .. 65535), so the hi and lo planes of an operand share one address register.
template <int OFF = 0>
__device__ inline s4v tr_read(uint32_t lds_addr) {
  static_assert(OFF >= 0 && OFF < 65536, "the offset must fit the DS offset field");
  s4v v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(lds_addr), "n"(OFF) : "memory");
  return v;
}
// One transposed fragment (8 reduction rows x 16 columns) from two such reads: a_lo / a_hi are this lane's LDS byte addresses
// of its two groups of 4 fragment rows, the lane's column part included.  tr_frag evaluates both addresses before the first
// read; where a kernel was tuned with the second address computed BEHIND the first read (read_frag below, resnet_stem.hip's
// weight gradient), it spells frag_join(tr_read(..), tr_read(..)) instead -- hipcc schedules the two forms differently.
__device__ inline bf8 frag_join(s4v lo, s4v hi) {
  const s8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf8, v);
}
template <int OFF = 0>
__device__ inline bf8 tr_frag(uint32_t a_lo, uint32_t a_hi) {
  const s4v lo = tr_read<OFF>(a_lo);
  const s4v hi = tr_read<OFF>(a_hi);
  return frag_join(lo, hi);
}
// every inline-asm LDS read issued so far has landed, and the compiler moves nothing across this point
__device__ inline void lds_reads_landed() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// ---- images of the LDS-DMA ring -------------------------------------------------------------------------------------------
// An operand tile sits in LDS as one of two lane-linear images, staged in 1 KiB pieces by glds16.  The chunk swizzle (16-byte
// chunks) is applied on the DMA source address by whoever stages the image and again by read_frag: both go through kc_sw / rc_sw.
//   KC ("k-contiguous", operand stored [r][k]): rows of 2*BK bytes, fragments by ds_read_b128.  The swizzle makes the lane
//      groups ({0-3,12-15,20-27}, ...) of a fragment read conflict-free: BK = 64: chunk ^ (row & 7); BK = 32 (4 chunks per row,
//      rows r, r+4, r+8, r+12 share their banks): chunk ^ (row & 8 ? 3 : 0).
//   RC ("r-contiguous", operand stored [k][r]): BK rows of 2*TB bytes, fragments by two transposed reads, so a transposed
//      operand never needs a transposed copy in HBM.  The swizzle keeps the 32-byte windows that the eight k-rows of a half-wave
//      read on distinct banks.
template <int BK>
__device__ inline int kc_sw(int row) { return BK == 64 ? (row & 7) : ((row & 8) ? 3 : 0); }
template <int BK>
__device__ inline int kc_off(int row, int chunk) { return row * (2 * BK) + 16 * (chunk ^ kc_sw<BK>(row)); }
template <int TB>
__device__ inline int rc_sw(int row) {
  return TB == 64 ? ((((row >> 1) & 1) | (((row >> 3) & 1) << 1)) << 1) : (((row & 3) << 2) | ((row >> 2) & 3));
}
template <int TB>
__device__ inline int rc_off(int row, int chunk) { return row * (TB * 2) + 16 * (chunk ^ rc_sw<TB>(row)); }

// fragment of the 16 rows/cols [rb, rb+16) x k-step s (32 deep) of the image at stage + OFF
template <bool KC, int TB, int BK, int OFF = 0>
__device__ inline bf8 read_frag(const char *stage, int rb, int s, int lane) {
  static_assert(OFF >= 0 && OFF < 65536, "image offset must fit the DS offset field");
  if (KC) {
    const int row = rb + (lane & 15);
    return *reinterpret_cast<const bf8 *>(stage + OFF + kc_off<BK>(row, 4 * s + (lane >> 4)));
  } else {
    const int g = lane >> 4, t = lane & 15, q = t >> 2, p = t & 3;
    const int row = 32 * s + 8 * g + q;
    const int chunk = (rb >> 3) + (p >> 1);
    const uint32_t base = lds_addr_of(stage);
    const s4v lo = tr_read<OFF>(base + rc_off<TB>(row, chunk) + 8 * (p & 1));
    const s4v hi = tr_read<OFF>(base + rc_off<TB>(row + 4, chunk) + 8 * (p & 1));
    return frag_join(lo, hi);
  }
}

}  // namespace crw
