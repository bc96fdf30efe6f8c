// Internal to the person detector's kernel translation units (det_*.hip; not seen by detnet.cpp,
// whose interface is det.h): the device helpers the kernel families share and the host helpers of
// their launchers.
#pragma once
#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "conv.h"
#include "det.h"
#include "mfma_tile.h"
#include "mvp_common.h"

namespace mvp {

// ---------------------------------------------------------------------------- device helpers
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
using mfma_tile::static_for;  // ring slots as compile-time register indices
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float bf(uint32_t v16) { return __uint_as_float(v16 << 16); }
__device__ __forceinline__ uint32_t tobf(float f) {
    __bf16 b = (__bf16)f;  // round to nearest even
    return (uint32_t)__builtin_bit_cast(uint16_t, b);
}
__device__ __forceinline__ float act_f(float v, int act) {
    if (act == 1) return fmaxf(v, 0.f);
    if (act == 2) return v * __builtin_amdgcn_rcpf(1.f + __expf(-v));  // v_exp + v_rcp (1 ulp): output is bf16
    return v;
}
__device__ __forceinline__ void unpack8(uint4 u, float* f) {
    f[0] = bf(u.x & 0xffff), f[1] = bf(u.x >> 16), f[2] = bf(u.y & 0xffff), f[3] = bf(u.y >> 16);
    f[4] = bf(u.z & 0xffff), f[5] = bf(u.z >> 16), f[6] = bf(u.w & 0xffff), f[7] = bf(u.w >> 16);
}
__device__ __forceinline__ uint4 pack8(const float* f) {
    return uint4{tobf(f[0]) | (tobf(f[1]) << 16), tobf(f[2]) | (tobf(f[3]) << 16), tobf(f[4]) | (tobf(f[5]) << 16),
                 tobf(f[6]) | (tobf(f[7]) << 16)};
}

// LDS-DMA of 16 B per lane: the wave's 64 lanes fill 1 KiB at lds_base in lane order
typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void gbl_void_t;
__device__ __forceinline__ void glds16_det(const void* src, void* lds_base) {
    __builtin_amdgcn_global_load_lds((gbl_void_t*)src, (lds_void_t*)lds_base, 16, 0, 0);
}

// s_waitcnt vmcnt(n') for the largest level n' <= n (wave-uniform n): at most n' of this
// wave's vector-memory operations stay outstanding (rounding down only waits longer)
__device__ __forceinline__ void wait_vm(int n) {
    if (n >= 24) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
    else if (n >= 20) asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
    else if (n >= 16) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if (n >= 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else if (n >= 10) asm volatile("s_waitcnt vmcnt(10)" ::: "memory");
    else if (n >= 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (n >= 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else if (n >= 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else if (n >= 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (n >= 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
    else if (n >= 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else if (n >= 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

__device__ __forceinline__ uint32_t lds_addr(const void* p) {
    typedef __attribute__((address_space(3))) const uint8_t lds_u8;
    return (uint32_t)(uintptr_t)(lds_u8*)p;
}
// LDS write / read-back of the epilogue staging as asm: the compiler would otherwise put a
// vmcnt(0) (the in-flight ring DMAs) in front of them; the read waits for the wave's writes
__device__ __forceinline__ void lds_write_u2(void* p, uint2 v) {
    asm volatile("ds_write_b64 %0, %1\n\ts_nop 1" : : "v"(lds_addr(p)), "v"(v) : "memory");
}
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
// raw buffer resource (stride 0, num_records bytes; gfx9 dword 3)
__device__ __forceinline__ i32x4 make_rsrc(const void* base, int bytes) {
    const uint64_t a = (uint64_t)(uintptr_t)base;
    return i32x4{__builtin_amdgcn_readfirstlane((int)(uint32_t)a), __builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32)),
                 __builtin_amdgcn_readfirstlane(bytes), 0x00020000};
}
// a weight-fragment load the compiler does not see (its waitcnt pass, seeing the LDS-DMAs and these
// loads as mixed event kinds, put vmcnt(0) in front of every third K step's MFMAs); the kernel's
// own end-of-step wait covers it
__device__ __forceinline__ bf16x8 buffer_load_frag(i32x4 r, int off) {
#ifdef PERS_BUILTIN_LOAD
    __amdgpu_buffer_rsrc_t rr;
    __builtin_memcpy(&rr, &r, 16);
    return __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rr, off, 0, 0));
#else
    bf16x8 v;
    // s_nop 4: the descriptor may be fresh from v_readfirstlane and the offset from a VALU op
    asm volatile("s_nop 4\n\tbuffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(v) : "v"(off), "s"(r) : "memory");
    return v;
#endif
}
// a buffer store the compiler does not see: its waitcnt pass would otherwise count it among the
// pending vector-memory events, see reads and writes mixed, and put vmcnt(0) in front of the next
// use of any load (the weight fragments two K steps ahead); the kernel's own waits count loads only
__device__ __forceinline__ void buffer_store_u4(u32x4 v, i32x4 r, int off) {
#ifdef PERS_BUILTIN_STORE
    __amdgpu_buffer_rsrc_t rr;
    __builtin_memcpy(&rr, &r, 16);
    __builtin_amdgcn_raw_buffer_store_b128(v, rr, off, 0, 0);
#else
    // s_nop 4 as the load; s_nop 1 after: the store reads its data registers late, and the
    // compiler's next instruction may overwrite them
    asm volatile("s_nop 4\n\tbuffer_store_dwordx4 %0, %1, %2, 0 offen\n\ts_nop 1" : : "v"(v), "v"(off), "s"(r) : "memory");
#endif
}
// this thread's two landed pixel chunks (16 B each) and their 4 scale quads in one wait (early
// clobber: a result register must not alias an address the later reads still need)
__device__ __forceinline__ void lds_read_ca6(const void* d0, const void* d1, const void* t0, const void* t1, u32x4& v0,
                                             u32x4& v1, f32x4& s00, f32x4& s01, f32x4& s10, f32x4& s11) {
    asm volatile(
        "ds_read_b128 %0, %6\n\tds_read_b128 %1, %7\n\tds_read_b128 %2, %8\n\tds_read_b128 %3, %8 offset:16\n\t"
        "ds_read_b128 %4, %9\n\tds_read_b128 %5, %9 offset:16\n\ts_waitcnt lgkmcnt(0)"
        : "=&v"(v0), "=&v"(v1), "=&v"(s00), "=&v"(s01), "=&v"(s10), "=&v"(s11)
        : "v"(lds_addr(d0)), "v"(lds_addr(d1)), "v"(lds_addr(t0)), "v"(lds_addr(t1))
        : "memory");
}
__device__ __forceinline__ void lds_write_u4(void* p, u32x4 v) {
    asm volatile("ds_write_b128 %0, %1\n\ts_nop 1" : : "v"(lds_addr(p)), "v"(v) : "memory");
}
__device__ __forceinline__ u32x4 lds_read_u4_sync(const void* p) {
    u32x4 v;
    asm volatile("s_waitcnt lgkmcnt(0)\n\tds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(lds_addr(p)) : "memory");
    return v;
}

// ds_read_b128 + its own lgkmcnt(0) in one asm block: the compiler cannot see it, so it inserts
// no vmcnt wait for the LDS-DMAs in flight (it assumes they may alias any LDS read it emits)
__device__ __forceinline__ float4 lds_read_f4_sync(const float* p) {
    typedef __attribute__((address_space(3))) float lds_float;
    const uint32_t a = (uint32_t)(uintptr_t)(const lds_float*)p;
    float4 v;
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
    return v;
}

// glds16_det to an LDS byte offset, as asm the compiler does not track (the persistent halo kernel
// counts its own waits)
__device__ __forceinline__ void glds16_raw(const void* src, uint32_t lds_off) {
    uint32_t saved;  // m0 is the compiler's: restored after the issue (the DMA reads it at issue)
    asm volatile("s_nop 4\n\ts_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(saved)
                 : "v"(src), "s"(lds_off)
                 : "memory");
}
__device__ __forceinline__ void buffer_store_u2v(u32x2 v, i32x4 r, int off) {
    asm volatile("s_nop 4\n\tbuffer_store_dwordx2 %0, %1, %2, 0 offen\n\ts_nop 1" : : "v"(v), "v"(off), "s"(r) : "memory");
}

}  // namespace

// ---------------------------------------------------------------------------- host helpers
// one workgroup per CU, a multiple of 8 (the XCD round robin of blockIdx)
DET_LOCAL inline int det_band_grid() { return det_cu_grid(cu_count()); }

// Grid of a persistent kernel over `items` work items with `occ` workgroups per CU: one workgroup
// per item, or a multiple of 8 (the kernels' per-XCD split needs one of the two)
DET_LOCAL inline long det_pers_grid(long items, long occ = 1) {
    const long cap = occ * det_band_grid();
    return items <= cap ? items : cap / 8 * 8;
}

// A runtime choice handed to a generic lambda as a constant (the launchers' template ladders)
template <int V>
using det_int = std::integral_constant<int, V>;

// Raises Kernel's dynamic-LDS limit to `bytes`, once per kernel function (call before a launch)
template <auto Kernel>
DET_LOCAL void det_dyn_lds(int bytes) {
    static const bool done = [bytes] {
        MVP_HIP(hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        return true;
    }();
    (void)done;
}

}  // namespace mvp
