/*
 * device_ops.hip.h -- the gfx950 primitives the kernels share: operand vector types, waits, wave-uniform values, LDS
 * offsets, LDS-DMA, raw LDS stores, buffer descriptors and the magic-reciprocal divide with its host-side reciprocals.
 *
 * Most of them are inline asm. hipcc treats an asm statement as one opaque instruction: it neither counts the memory
 * operations inside it (no s_waitcnt is emitted for them) nor pads their hazards (cdna_hip_programming.md section 5.7).
 * Every asm primitive below says who waits for it; the caller does that waiting.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

namespace qnnp {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

// nothing is scheduled across this point
#define QNNP_PIN() __builtin_amdgcn_sched_barrier(0)

template <int N>
__device__ __forceinline__ void wait_vmcnt()
{
  static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit field");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

/* A wave-uniform value, in scalar registers for good. A uniform value the compiler happened to compute with vector
 * instructions -- a 64-bit multiply, say -- would reach an "s" asm operand as a VGPR pair: an assembler error. */
__device__ __forceinline__ uint64_t scalar_ptr(uint64_t v)
{
  const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v));
  const uint32_t hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
  return (static_cast<uint64_t>(hi) << 32) | lo;
}
__device__ __forceinline__ const uint8_t* scalar_ptr(const uint8_t* ptr)
{
  return reinterpret_cast<const uint8_t*>(scalar_ptr(reinterpret_cast<uint64_t>(ptr)));
}

// byte offset of an LDS pointer inside the workgroup's LDS allocation (what DS instructions and M0 address)
__device__ __forceinline__ uint32_t lds_offset(const void* p)
{
  return static_cast<uint32_t>(reinterpret_cast<uintptr_t>((const __attribute__((address_space(3))) uint8_t*) p));
}

/*
 * LDS-DMA (global_load_lds_dwordx4): 16 bytes per lane from global memory to LDS at M0 + lane * 16, M0 being the
 * wave-uniform LDS destination of lane 0. The data lands in LDS behind the wave's vmcnt: the caller waits with
 * wait_vmcnt, then a barrier, before any wave reads it (__syncthreads alone does not wait for it).
 *
 * Why inline asm and not __builtin_amdgcn_global_load_lds (dma16_builtin below): with the builtin, hipcc (ROCm 7.2)
 * remembers that a global_load_lds is in flight and puts s_waitcnt vmcnt(0) in front of every later LDS access it cannot
 * prove disjoint -- inside a unit loop that is every ds_read / ds_write / LDS atomic, each draining the loads meant to
 * land under the work that runs meanwhile. The asm forms are invisible to that bookkeeping; the only waits are the
 * caller's explicit ones. And for a wave-uniform 64-bit base plus a 32-bit lane offset, hipcc selects the VGPR-pair
 * address form for the builtin whatever the shape of the address expression (one v_lshl_add_u64 per piece); the saddr
 * forms below issue the SGPR-base instruction itself.
 *
 * M0 is a register the compiler reserves; it does not preserve it around an asm statement and ignores it in a clobber
 * list. Hence M0 is written in the statement that reads it, and the forms differ in who owns it afterwards:
 * dma16_flat_keep_m0 restores it; the other asm forms leave it written, which only a kernel in which nothing else reads
 * M0 may use (tests/test_kernel_resources.py disassembles those kernels and checks). The s_nop 0 is the wait state
 * between the M0 write and the load.
 *
 * The forms with a "memory" clobber keep the compiler's own loads and stores on their side of the statement; the GEMMs'
 * saddr forms have none.
 */

/* flat per-lane source, M0 saved and restored: for kernels in which the compiler also uses M0 */
__device__ __forceinline__ void dma16_flat_keep_m0(const uint8_t* src, uint8_t* lds_wave_base)
{
  const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_offset(lds_wave_base));
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep) : "v"(src), "s"(dst) : "memory");
}

/* flat per-lane source, M0 written and left, "memory" clobber; lds_dst: LDS byte offset, made wave-uniform here */
__device__ __forceinline__ void dma16_flat(const uint8_t* src, uint32_t lds_dst)
{
  const uint32_t dst = __builtin_amdgcn_readfirstlane(lds_dst);
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(src), "s"(dst) : "memory");
}

/* saddr form (wave-uniform 64-bit base in an SGPR pair + 32-bit lane offset), M0 written and left, no clobber */
__device__ __forceinline__ void dma16_saddr(const uint8_t* base, uint32_t lane_offset, uint8_t* lds_wave_base)
{
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
               : : "v"(lane_offset), "s"(base), "s"(lds_offset(lds_wave_base)));
}

/* saddr form, M0 written and left, "memory" clobber; base and lds_dst (an LDS byte offset) must already be scalar */
__device__ __forceinline__ void dma16_saddr_ordered(uint64_t base, uint32_t lane_offset, uint32_t lds_dst)
{
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(lane_offset), "s"(base), "s"(lds_dst) : "memory");
}

/* The saddr form in two halves, for a main loop: dma16_set_m0 writes M0 one instruction (an MFMA) ahead of the load,
 * which is the wait state the pair needs (no s_nop); dma16_saddr_m0_set then issues the load. Nothing else in that loop
 * may touch M0. No clobbers. */
__device__ __forceinline__ void dma16_set_m0(uint8_t* lds_wave_base)
{
  asm volatile("s_mov_b32 m0, %0" : : "s"(lds_offset(lds_wave_base)));
}
__device__ __forceinline__ void dma16_saddr_m0_set(const uint8_t* base, uint32_t lane_offset)
{
  asm volatile("global_load_lds_dwordx4 %0, %1" : : "v"(lane_offset), "s"(base));
}

/* The builtin, flat per-lane source. The compiler sets M0 and counts the load (with the vmcnt(0) guards above).
 * QNNP_DMA_AUX: its cache-policy bits, an A/B knob at build time (make EXTRA=-DQNNP_DMA_AUX=...). */
#ifndef QNNP_DMA_AUX
#define QNNP_DMA_AUX 0
#endif
__device__ __forceinline__ void dma16_builtin(const uint8_t* src, uint8_t* lds_wave_base)
{
  __builtin_amdgcn_global_load_lds(
      (const __attribute__((address_space(1))) void*) src,
      (__attribute__((address_space(3))) void*) lds_wave_base, 16, 0, QNNP_DMA_AUX);
}

/* 16-byte / 4-byte LDS stores the compiler does not see as LDS accesses: no vmcnt(0) in front of them for an LDS-DMA in
 * flight. Their completion is the caller's to wait for (lgkmcnt, or a barrier). */
__device__ __forceinline__ void ds_write16(uint32_t off, v4i x)
{
  asm volatile("ds_write_b128 %0, %1" :: "v"(off), "v"(x) : "memory");
}
__device__ __forceinline__ void ds_write16(uint32_t off, uint4 v)
{
  const v4i x = {static_cast<int>(v.x), static_cast<int>(v.y), static_cast<int>(v.z), static_cast<int>(v.w)};
  ds_write16(off, x);
}
__device__ __forceinline__ void ds_write4(uint32_t off, int32_t v)
{
  asm volatile("ds_write_b32 %0, %1" :: "v"(off), "v"(v) : "memory");
}

/* Buffer descriptor over `bytes` bytes from ptr (stride 0: the record count is in bytes; a lane whose offset lies past
 * it reads zeros and its store is dropped). Build it from wave-uniform values only. */
constexpr int kBufferRsrcFlags = 0x00020000;   // descriptor word 3: DATA_FORMAT (bits 18:15) = 4, 32-bit; all else 0
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* ptr, int bytes)
{
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(ptr), 0, bytes, kBufferRsrcFlags);
}

/* chunk swizzle of the GEMMs' activation image: rows 8..15 of every 16 keep their K chunks in slots c ^ 3 */
__device__ __forceinline__ uint32_t a_swizzle(uint32_t row) { return (row & 8u) != 0 ? 3u : 0u; }

/*
 * n / d by a host-made reciprocal: one scalar multiply instead of the ~40-instruction sequence hipcc emits for a
 * division by a run-time value. inv == 0 stands for d == 1. The two host formulas below give different values (for a
 * power of two d, say); each kernel was checked with the one its launcher uses.
 */
__device__ __forceinline__ uint32_t div_magic(uint32_t n, uint32_t inv) { return inv != 0u ? __umulhi(n, inv) : n; }

/* ceil(2^32 / d), 0 for d <= 1: div_magic(n, .) == n / d for n * d < 2^32 (error term n * e / (d * 2^32) < 1 / d) */
inline uint32_t reciprocal_ceil(uint32_t d)
{
  return d > 1 ? static_cast<uint32_t>(((UINT64_C(1) << 32) + d - 1) / d) : 0u;
}

/* floor(2^32 / d) + 1, for d >= 2: div_magic(n, .) == n / d for n * d < 2^32. (d == 1 wraps to 1, which divides
 * nothing: callers that can meet it pass 0 instead.) */
inline uint32_t reciprocal_floor_plus1(uint32_t d) { return static_cast<uint32_t>((UINT64_C(1) << 32) / d) + 1u; }

}  // namespace qnnp
