// The split operand image: how every convolution on the hot path reads its activations, and the one place that says so.
// THE LAYOUT.  An activation x [K][N] (K channels = the GEMM's k, N columns) is stored as fp16 [kbx(K)][p * 2 + kh][N + 1][8]:
//   k-block kb = k / 16 (kbx(K) of them: the blocks of K rounded up to a multiple of 4, a 64-row block of the reader's k loop),
//   part p: x = h + l to 22 bits, p = 0 the fp16 nearest to x, p = 1 the fp16 nearest to the exact remainder x - h,
//   k-half kh = (k / 8) % 2, then the column, then the 8 consecutive k of the half: one ROW of 16 bytes.
// So an 8-row group g = k / 8 = 2 kb + kh owns the two PLANES kb * 4 + kh (h) and kb * 4 + kh + 2 (l), a plane is N + 1 rows, and the l
// row of a value lies two planes = 2 (N + 1) rows behind its h row.
//   The zero column.  Column N of every plane is zero: the reader points a tap that falls outside the utterance at it.
//   The zero rows.  Rows k >= K, up to 16 kbx(K), are zero in every column: the reader's k loop runs over whole 64-row blocks.
// A writer owns both rules for the groups it writes; g < 2 kbx(K) bounds the groups.  Plain C++17 (tests/test_operand_image_cpu.py holds
// the index functions to oracle/gemm_ref.py: image_parts with g++); the device half -- the split and the row stores -- is behind __HIPCC__.
#pragma once
#include <cstddef>
#include <cstdint>

namespace operand_image {
#ifdef __HIPCC__
#define OI_HD __host__ __device__ __forceinline__
#else
#define OI_HD
#endif
// k-blocks of an image of K rows: a multiple of 4
OI_HD constexpr int kbx(int K) { return (((K + 15) >> 4) + 3) & ~3; }
// rows of a plane of N columns + the zero column: NX below (formed once by the caller: inside every function hipcc folds each N + 1 apart)
OI_HD constexpr size_t rows(int N) { return (size_t)N + 1; }
OI_HD constexpr unsigned rows32(int N) { return (unsigned)N + 1u; }
// bytes of the image of x [K][N] (nothing for an empty one)
OI_HD constexpr size_t bytes(int K, int N) { return K <= 0 || N <= 0 ? 0 : (size_t)kbx(K) * 4 * rows(N) * 16; }
// the same for a buffer descriptor (32-bit: the hosts check the image against 2 GiB), of an image that is there; kb = its k-blocks
OI_HD constexpr unsigned desc_bytes_kb(int kb, unsigned NX) { return (unsigned)kb * 4u * NX * 16u; }
OI_HD constexpr unsigned desc_bytes(int K, unsigned NX) { return desc_bytes_kb(kbx(K), NX); }
// plane of (k-block kb, part p, k-half kh), and of 8-row group g = 2 kb + kh, part p (an LDS tile may keep this order at its own stride)
template <typename T>
OI_HD constexpr T plane_of(T kb, int p, int kh) { return kb * 4 + p * 2 + kh; }
OI_HD constexpr int plane(int g, int p = 0) { return (g >> 1) * 4 + (g & 1) + 2 * p; }
// 16-byte row of (g, p, column j) in an image of NX rows to a plane, and of column j of a plane
OI_HD constexpr size_t plane_row(size_t pl, size_t j, size_t NX) { return pl * NX + j; }
OI_HD constexpr size_t row_of(int kb, int p, int kh, size_t j, size_t NX) { return plane_row(plane_of((size_t)kb, p, kh), j, NX); }
OI_HD constexpr size_t row(int g, int p, size_t j, size_t NX) { return plane_row((size_t)(g >> 1) * 4 + (g & 1) + 2 * p, j, NX); }
// ... as a byte offset for the buffer-descriptor writers
OI_HD constexpr unsigned byte_off(int pl, unsigned j, unsigned NX) { return ((unsigned)pl * NX + j) * 16u; }   // pl = plane / plane_of
#undef OI_HD
}  // namespace operand_image
#ifdef __HIPCC__
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));
// two fp32 -> (h, l) fp16 pairs with x = h + l to 22 bits: v_cvt_pk_f16_f32 (RNE), the residual is exact in fp32
static __device__ __forceinline__ void split2_pair(float x0, float x1, unsigned& h, unsigned& l)
{
    const f32x2 v = {x0, x1};
    const f16x2 hh = __builtin_convertvector(v, f16x2);
    const f32x2 r = v - __builtin_convertvector(hh, f32x2);
    h = __builtin_bit_cast(unsigned, hh);
    l = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
}
// 8 fp32 (consecutive k of one column) -> two 16-byte rows of 8 fp16
static __device__ __forceinline__ void split2(const float (&x)[8], u32x4_t& h, u32x4_t& l)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        unsigned hu, lu;
        split2_pair(x[2 * e], x[2 * e + 1], hu, lu);
        h[e] = hu;
        l[e] = lu;
    }
}
// one value's two rows: h at row `at` (operand_image::row of part 0), l two planes on.  NX = operand_image::rows(N) here and below
static __device__ __forceinline__ void oi_store(u32x4_t* img, size_t at, size_t NX, u32x4_t h, u32x4_t l)
{
    img[at] = h;
    img[at + 2 * NX] = l;
}
static __device__ __forceinline__ void oi_store(u32x4_t* img, size_t at, size_t NX, const float (&x)[8])
{
    u32x4_t h, l;
    split2(x, h, l);
    oi_store(img, at, NX, h, l);
}
// the same through a buffer descriptor: off = operand_image::byte_off of the h plane, or the caller's out-of-range offset (both stores dropped)
static __device__ __forceinline__ void oi_store_buf(__amdgpu_buffer_rsrc_t rs, unsigned off, unsigned NXy, u32x4_t h, u32x4_t l)
{
    __builtin_amdgcn_raw_buffer_store_b128(h, rs, off, 0, 0);
    __builtin_amdgcn_raw_buffer_store_b128(l, rs, off + 2u * NXy * 16u, 0, 0);
}
static __device__ __forceinline__ void oi_store_buf(__amdgpu_buffer_rsrc_t rs, unsigned off, unsigned NXy, const float (&x)[8])
{
    u32x4_t h, l;
    split2(x, h, l);
    oi_store_buf(rs, off, NXy, h, l);
}
// the zero column N of a group, both parts or part p alone (a thread per part); plane0 = operand_image::row of its h plane's column 0
static __device__ __forceinline__ void oi_zero_column(u32x4_t* img, size_t plane0, size_t N, size_t NX)
{
    img[plane0 + N] = u32x4_t{0u, 0u, 0u, 0u};
    img[plane0 + 2 * NX + N] = u32x4_t{0u, 0u, 0u, 0u};
}
static __device__ __forceinline__ void oi_zero_column(u32x4_t* img, size_t plane0, size_t p, size_t N, size_t NX) { img[plane0 + p * 2 * NX + N] = u32x4_t{0u, 0u, 0u, 0u}; }
#endif
