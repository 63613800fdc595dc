// The hand-synchronised gfx950 primitives: LDS access from inline assembly, LDS-DMA, counted waits, stamps.
// Every kernel that places its own s_waitcnt is built from these; each primitive has ONE definition, here.
//
// The rules (each learnt from a wrong result or a measured stall):
//  1. Inside a loop that keeps LDS-DMA in flight, EVERY LDS access is inline asm (lds_read_tr / lds_read16 /
//     lds_write*). hipcc orders each ds_read / ds_write it can see behind all pending LDS-DMA with s_waitcnt
//     vmcnt(0) -- it cannot tell the stage being filled from the stage being read -- which drains the chunks in
//     flight once per chunk (gemm_wgrad_full.cuh; cconv_dma.cuh; conv_nhwc.hip). A DMA it can see (dccrn.hip), a
//     second __shared__ object or run-time stage numbers (gemm_wgrad_full.cuh) do the same. The waits are placed
//     by hand: wait_vm<N> retires the older DMAs, wait_lgkm<N> the LDS reads. lds_read_tr_tracked is the other
//     kind, a builtin the compiler waits for by itself, for kernels WITHOUT pending DMA: not interchangeable.
//  2. The result of an asm LDS read is valid only behind a wait_lgkm that names it, and the tie is on the WHOLE
//     vector: with a per-component tie the compiler may copy a component out (or move, or spill the register)
//     BEFORE the wait, i.e. before the data arrived (gemm_wgrad_full.cuh; the back edge of conv_nhwc.hip's loop).
//  3. DS operations return in order, and so do a wave's vector-memory operations: wait_lgkm<N> / wait_vm<N> prove
//     every operation except the N youngest (hipcc's own counted waits rely on it).
//  4. A load in flight that the compiler does not know about has NO register destination: LDS-DMA only. The
//     recurrences of rounds 4 - 5 prefetched by global_load_dword from inline assembly behind a counted vmcnt; a
//     phi copy of the rotating register sets (`v_mov_b32 v135, v136` one step after `global_load_dword v136`,
//     before its wait) read the destination whether or not the load had landed: under HBM load one run in three of
//     tests/test_gpu_sizes.py::test_dccrn_default_size_gradients_fp32_and_use_amp had LSTM gradients 10^3 off
//     (profiles/r06_lstm_race.txt). A counted vmcnt that releases TRACKED loads (lstm_tile.hip) is tied as in 2.
//  5. m0 belongs to dma4_m0: a kernel that uses it contains no other user of m0.
//
// Asm that deliberately stays in the kernels:
//  * multi-instruction batches that are one scheduling unit (lstm_read4 in dccrn.hip, the WD_FRAGS / WD_MFMAS
//    macros and the read + wait of keep_first in cconv_wgrad_dma.cuh, the 16 ds_read_b32 + wait of conv_nhwc.hip's
//    statistics);
//  * the empty-template register pins, asm volatile("" : "+v"(x));
//  * the opaque scalar move of conv_nhwc.hip's tap body;
//  * the ablation branches of diagnostic builds.
#pragma once
#include "common.cuh"

namespace brv {

typedef __attribute__((address_space(3))) void* lds_void_p;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_p;
typedef __attribute__((address_space(1))) const void* glb_void_p;

// low 32 bits of a flat LDS address = the address ds_* instructions take
__device__ __forceinline__ unsigned int lds_addr(const void* p) { return (unsigned int)(unsigned long long)p; }

// ---- LDS reads / writes the compiler cannot see (rule 1); a read is valid behind its wait_lgkm (rule 2) ------
// OFF is the instruction's 16-bit immediate. Transposing read: 4 rows x 16 columns (16-bit) per 16-lane group, delivered column-major
template <int OFF = 0>
__device__ __forceinline__ s16x4 lds_read_tr(unsigned int addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
  s16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
// the same read as a builtin on a flat pointer into LDS: compiler-tracked (its own lgkmcnt, and vmcnt(0) first
// when DMAs are pending: rule 1)
__device__ __forceinline__ s16x4 lds_read_tr_tracked(const void* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_p)p);
}
template <int OFF = 0>
__device__ __forceinline__ u32x4 lds_read16(unsigned int addr) {
  static_assert(OFF >= 0 && OFF < 65536, "ds offset field");
  u32x4 v;
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
  return v;
}
__device__ __forceinline__ void lds_write16(unsigned int addr, const u32x4& v) {
  asm volatile("ds_write_b128 %0, %1" :: "v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_write16(unsigned int addr, const uint4& q) {
  u32x4 v; v.x = q.x; v.y = q.y; v.z = q.z; v.w = q.w;
  lds_write16(addr, v);
}
template <class V>
__device__ __forceinline__ void lds_write8(unsigned int addr, const V& v) {
  static_assert(sizeof(V) == 8, "8-byte vector");
  asm volatile("ds_write_b64 %0, %1" :: "v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void lds_write2(unsigned int addr, unsigned int v) {      // the low 16 bits of v
  asm volatile("ds_write_b16 %0, %1" :: "v"(addr), "v"(v) : "memory");
}

// ---- global -> LDS DMA: no VGPR round trip, no register destination (rule 4); counted by vmcnt ---------------
// buffer descriptor, 16 bytes per lane: LDS destination `dst` (wave-uniform) + lane*16, source r + voff (per
// lane); pieces outside the descriptor arrive as zeros
__device__ __forceinline__ void dma16_buf(__amdgpu_buffer_rsrc_t r, unsigned char* dst, unsigned int voff) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_p)dst, 16, (int)voff, 0, 0, 0);
}
// flat pointer per lane, 16 bytes per lane, same destination rule
__device__ __forceinline__ void dma16_flat(const void* g, unsigned char* dst) {
  __builtin_amdgcn_global_load_lds((glb_void_p)g, (lds_void_p)dst, 16, 0, 0);
}
// one dword per lane through m0: lane l writes LDS byte address `lds_wave_base` (wave-uniform) + 4 l. Assembly,
// so that the compiler sees no DMA (rule 1); m0 has no other user (rule 5).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
__device__ __forceinline__ void dma4_m0(const float* lane_src, unsigned int lds_wave_base) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off"
               :: "v"(lane_src), "s"(lds_wave_base) : "memory", "m0");
}
#pragma clang diagnostic pop

// ---- counted waits (rule 3) ----------------------------------------------------------------------------------
// at most N vector-memory operations (loads, stores, DMAs) of this wave are still pending
template <int N>
__device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory"); }
// ... and the registers named are the destinations of TRACKED loads this wait releases (rule 4)
template <int N, class A>
__device__ __forceinline__ void wait_vm(A& a) { asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(N) : "memory"); }
template <int N, class A, class B, class C, class D>
__device__ __forceinline__ void wait_vm(A& a, B& b, C& c, D& d) {
  asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N) : "memory");
}
// at most N LDS operations are still pending: the registers named (whole vectors: rule 2) are valid from here
template <int N>
__device__ __forceinline__ void wait_lgkm() { asm volatile("s_waitcnt lgkmcnt(%0)" :: "n"(N) : "memory"); }
template <int N, class A>
__device__ __forceinline__ void wait_lgkm(A& a) { asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(N) : "memory"); }
template <int N, class A, class B>
__device__ __forceinline__ void wait_lgkm(A& a, B& b) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory");
}
template <int N, class A, class B, class C, class D>
__device__ __forceinline__ void wait_lgkm(A& a, B& b, C& c, D& d) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N) : "memory");
}
template <int N, class A, class B, class C, class D, class E>
__device__ __forceinline__ void wait_lgkm(A& a, B& b, C& c, D& d, E& e) {
  asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e) : "n"(N) : "memory");
}
template <int N, class A, class B, class C, class D, class E, class F>
__device__ __forceinline__ void wait_lgkm(A& a, B& b, C& c, D& d, E& e, F& f) {
  asm volatile("s_waitcnt lgkmcnt(%6)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f) : "n"(N) : "memory");
}
template <int N, class A, class B, class C, class D, class E, class F, class G, class H, class I, class J>
__device__ __forceinline__ void wait_lgkm(A& a, B& b, C& c, D& d, E& e, F& f, G& g, H& h, I& i, J& j) {
  asm volatile("s_waitcnt lgkmcnt(%10)"
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(f), "+v"(g), "+v"(h), "+v"(i), "+v"(j)
               : "n"(N) : "memory");
}
// Workgroup barrier that orders LDS traffic only: this wave's LDS operations complete, then s_barrier.
// __syncthreads() also waits for every global access in flight (vmcnt(0) counts loads AND stores on gfx9).
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// ---- stamps of diagnostic builds -----------------------------------------------------------------------------
// (scalar-memory instructions: the result is in its registers only behind lgkmcnt(0))
__device__ __forceinline__ long long stamp_cycles() {        // s_memtime
  long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
  return t;
}
__device__ __forceinline__ long long stamp_realtime() {      // s_memrealtime: the 100 MHz constant clock
  long long t;
  asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) :: "memory");
  return t;
}

}  // namespace brv
