// mfma_types.h -- the vector types of the MFMA kernels and the bf16 primitives more than one file uses (device code only).
#pragma once
#include <cstdint>

namespace ampnet {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
#if defined(__HIPCC__) || defined(__HIP__)
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

// index of window q's per-window parameters (PwGemm / PwBwd .perwin_slot_major)
__device__ __forceinline__ int pidx_of(int q, int n_slots, int Q, int slot_major)
{
    return slot_major ? (q % n_slots) * (Q / n_slots) + q / n_slots : q;
}

// ---- fp32 -> bf16, rounded once ----
__device__ __forceinline__ bf16x4 to_bf16x4(const f32x4 &v)
{
    bf16x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (__bf16)v[i];       // v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN
    return o;
}
__device__ __forceinline__ bf16x8 pack_bf16(const f32x4 &lo, const f32x4 &hi)
{
    bf16x8 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        o[i] = (__bf16)lo[i];
        o[4 + i] = (__bf16)hi[i];
    }
    return o;
}

// ---- Three-term bf16 split (precision mode AMPNET_PRECISION_F32_SPLIT) ----
// x = p1 + p2 + p3 exactly -- p1 = bf16(x), p2 = bf16(x - p1), p3 = bf16(x - p1 - p2), round to nearest even each time; the residual of an
// fp32 number against its 8-bit head has at most 16 significant bits, the second residual at most 8, so both subtractions and the last
// conversion are exact.  Written on PAIRS so that it compiles to v_cvt_pk_bf16_f32 + (shift, and) + v_pk_add_f32 per step: 9 VALU
// instructions per two elements.
__device__ __forceinline__ uint32_t cvt_pk_bf16(const f32x2 &v)
{
    // as an instruction, not as two conversions: written in C the optimiser re-converts a lone element wherever only one half of the
    // pair is needed again (the residuals below), 13 conversions per eight elements instead of 12 and scalar subtractions instead of packed
    uint32_t p;
    asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(p) : "v"(v[0]), "v"(v[1]));
    return p;
}
__device__ __forceinline__ f32x2 widen_pk_bf16(uint32_t p)
{
    return f32x2{__builtin_bit_cast(float, p << 16), __builtin_bit_cast(float, p & 0xffff0000u)};
}
__device__ __forceinline__ void split3_pair(const f32x2 &x, uint32_t &p1, uint32_t &p2, uint32_t &p3)
{
    p1 = cvt_pk_bf16(x);
    const f32x2 r = x - widen_pk_bf16(p1);
    p2 = cvt_pk_bf16(r);
    p3 = cvt_pk_bf16(r - widen_pk_bf16(p2));
}
__device__ __forceinline__ void split3_bf16(const f32x4 &v, bf16x4 &p1, bf16x4 &p2, bf16x4 &p3)
{
    uint32_t q1[2], q2[2], q3[2];
    split3_pair(f32x2{v[0], v[1]}, q1[0], q2[0], q3[0]);
    split3_pair(f32x2{v[2], v[3]}, q1[1], q2[1], q3[1]);
    p1 = __builtin_bit_cast(bf16x4, u32x2{q1[0], q1[1]});
    p2 = __builtin_bit_cast(bf16x4, u32x2{q2[0], q2[1]});
    p3 = __builtin_bit_cast(bf16x4, u32x2{q3[0], q3[1]});
}
__device__ __forceinline__ void split3_bf16(const f32x4 &lo, const f32x4 &hi, bf16x8 &p1, bf16x8 &p2, bf16x8 &p3)
{
    uint32_t q1[4], q2[4], q3[4];
    split3_pair(f32x2{lo[0], lo[1]}, q1[0], q2[0], q3[0]);
    split3_pair(f32x2{lo[2], lo[3]}, q1[1], q2[1], q3[1]);
    split3_pair(f32x2{hi[0], hi[1]}, q1[2], q2[2], q3[2]);
    split3_pair(f32x2{hi[2], hi[3]}, q1[3], q2[3], q3[3]);
    p1 = __builtin_bit_cast(bf16x8, u32x4{q1[0], q1[1], q1[2], q1[3]});
    p2 = __builtin_bit_cast(bf16x8, u32x4{q2[0], q2[1], q2[2], q2[3]});
    p3 = __builtin_bit_cast(bf16x8, u32x4{q3[0], q3[1], q3[2], q3[3]});
}
__device__ __forceinline__ void split3_bf16(const float (&v)[8], bf16x8 &p1, bf16x8 &p2, bf16x8 &p3)      // eight scalars gathered one by one
{
    split3_bf16(f32x4{v[0], v[1], v[2], v[3]}, f32x4{v[4], v[5], v[6], v[7]}, p1, p2, p3);
}

// MFMA operand whose k runs over the ROWS of a row-major bf16 tile: rows row0 .. row0 + 15, channel col0 + (lane & 31).
// EXEC must be all ones (the read gathers across lanes): only called from wave-uniform code.
__device__ __forceinline__ bf16x8 tr_operand(const __bf16 *tile, int ld, int row0, int col0, int lane)
{
    const int g4 = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
    const __bf16 *src = tile + (row0 + 8 * (g4 >> 1) + q) * ld + col0 + 16 * (g4 & 1) + 4 * p;
    typedef s16x4 __attribute__((address_space(3))) * lds_ptr;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(src));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(src + 4 * ld));
    // whole-vector bit casts + one shuffle: an element-by-element short -> __bf16 copy is miscompiled by this hipcc (ROCm 7.2: it keeps
    // only the first dword of each read; tools/tr_probe.hip checks the operand map on the hardware)
    return __builtin_shufflevector(__builtin_bit_cast(bf16x4, lo), __builtin_bit_cast(bf16x4, hi), 0, 1, 2, 3, 4, 5, 6, 7);
}
#endif

}  // namespace ampnet
