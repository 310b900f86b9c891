// fe_pixfmt_dev.h — the per-lane arithmetic of lvk_image_to_gray (fe_pixfmt.hip; contract in include/lvk_c.h), as __host__ __device__
// functions: the kernel calls pixfmt_lane once per lane, and tests/host/pixfmt_check.hip runs the very same function on the CPU under
// AddressSanitizer, every source row in a heap block of its own, so a read past a row is a report there and not a guess here.
//
// One lane owns one ALIGNED dword of the destination row: lane k of a row whose first byte sits `off` = (address & 3) bytes into a
// dword covers the pixels [4k - off, 4k - off + 4), clipped to [0, w).  A lane with all four pixels stores one dword, the clipped
// lanes at either end of the row store bytes: nothing outside dst[0 .. w) is written.  The source bytes of those pixels are one
// contiguous run of 4 * bytes_per_pixel bytes; a full lane whose run starts on a dword boundary loads it as dwords (they lie inside the
// row by construction: nothing is rounded outward), every other lane loads bytes - and only the bytes of its own pixels.
#pragma once
#include <stdint.h>
#include "../../include/lvk_c.h"

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif
#endif

#if defined(__BYTE_ORDER__) && __BYTE_ORDER__ != __ORDER_LITTLE_ENDIAN__
#error "fe_pixfmt_dev.h assembles dwords from bytes in little-endian order (x86-64 hosts, gfx950)"
#endif

// Hook of the host harness: called with every address range a lane is about to load (kind 0) or store (kind 1).  AddressSanitizer sees
// a byte past the END of a heap block but cannot see one in front of a row that does not start on its 8-byte granule; the harness
// records the ranges instead and holds them to the row.  Nothing in the library.
#ifndef PIXFMT_TOUCH
#define PIXFMT_TOUCH(kind, ptr, nbytes) do { } while (0)
#endif

// bytes per pixel of a format; 0 = not a format
__host__ __device__ inline int lvk_pixfmt_bpp(int format)
{
    switch (format) {
    case LVK_PIX_MONO8: return 1;
    case LVK_PIX_BGR8: case LVK_PIX_RGB8: return 3;
    case LVK_PIX_BGRA8: case LVK_PIX_RGBA8: return 4;
    case LVK_PIX_MONO16: case LVK_PIX_YUYV: case LVK_PIX_UYVY: return 2;
    default: return 0;
    }
}
inline const char* lvk_pixfmt_name(int format)
{
    static const char* const names[] = {"mono8", "bgr8", "rgb8", "bgra8", "rgba8", "mono16", "yuyv", "uyvy"};
    return format >= 0 && format < 8 ? names[format] : "?";
}

// the colour formula of the contract: integers, weights sum to 2^14, so (g, g, g) -> g and the result stays in 0..255
__host__ __device__ inline unsigned pixfmt_bgr_to_gray(unsigned b, unsigned g, unsigned r)
{
    return (1868u * b + 9617u * g + 4899u * r + 8192u) >> 14;
}

// byte j of a run held as little-endian dwords
__host__ __device__ inline unsigned pixfmt_byte(const uint32_t* v, int j) { return (v[j >> 2] >> (8 * (j & 3))) & 255u; }

// grey of pixel i of the run v (pixel i's bytes start at byte i * bpp)
template <int FMT>
__host__ __device__ inline unsigned pixfmt_pixel(const uint32_t* v, int i, int shift)
{
    if (FMT == LVK_PIX_MONO8) return pixfmt_byte(v, i);
    if (FMT == LVK_PIX_BGR8)  return pixfmt_bgr_to_gray(pixfmt_byte(v, 3 * i), pixfmt_byte(v, 3 * i + 1), pixfmt_byte(v, 3 * i + 2));
    if (FMT == LVK_PIX_RGB8)  return pixfmt_bgr_to_gray(pixfmt_byte(v, 3 * i + 2), pixfmt_byte(v, 3 * i + 1), pixfmt_byte(v, 3 * i));
    if (FMT == LVK_PIX_BGRA8) return pixfmt_bgr_to_gray(pixfmt_byte(v, 4 * i), pixfmt_byte(v, 4 * i + 1), pixfmt_byte(v, 4 * i + 2));
    if (FMT == LVK_PIX_RGBA8) return pixfmt_bgr_to_gray(pixfmt_byte(v, 4 * i + 2), pixfmt_byte(v, 4 * i + 1), pixfmt_byte(v, 4 * i));
    if (FMT == LVK_PIX_MONO16) {
        const unsigned s = ((v[i >> 1] >> (16 * (i & 1))) & 0xFFFFu) >> shift;
        return s > 255u ? 255u : s;
    }
    if (FMT == LVK_PIX_YUYV) return pixfmt_byte(v, 2 * i);
    return pixfmt_byte(v, 2 * i + 1);                        // LVK_PIX_UYVY
}

template <int FMT> struct PixfmtBpp { static const int value = FMT == LVK_PIX_MONO8 ? 1 : (FMT == LVK_PIX_BGR8 || FMT == LVK_PIX_RGB8) ? 3 : (FMT == LVK_PIX_BGRA8 || FMT == LVK_PIX_RGBA8) ? 4 : 2; };

// lanes a row needs: the aligned dwords that dst_row[0 .. w) touches
__host__ __device__ inline int pixfmt_row_lanes(const uint8_t* dst_row, int w) { return (int)((((uintptr_t)dst_row & 3u) + (unsigned)w + 3u) >> 2); }

// Lane k of one row (0 <= k < pixfmt_row_lanes; a k beyond that does nothing).  src_row: first byte of the source row, w * bpp bytes
// readable; dst_row: first byte of the destination row, w bytes writable.
template <int FMT>
__host__ __device__ inline void pixfmt_lane(const uint8_t* src_row, uint8_t* dst_row, int w, int shift, int k)
{
    constexpr int BPP = PixfmtBpp<FMT>::value;
    const int off = (int)((uintptr_t)dst_row & 3u);
    const int xa = 4 * k - off;                              // pixel of the lane's dword byte 0 (may be < 0 in lane 0)
    const int x0 = xa < 0 ? 0 : xa, x1 = xa + 4 > w ? w : xa + 4;
    if (x0 >= x1) return;
    const bool full = x1 - x0 == 4;                          // then x0 == xa and dst_row + x0 is dword-aligned
    const uint8_t* s = src_row + (size_t)x0 * BPP;
    uint32_t v[BPP] = {};
    if (full && ((uintptr_t)s & 3u) == 0) {
        const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
        PIXFMT_TOUCH(0, s4, 4 * BPP);
#pragma unroll
        for (int j = 0; j < BPP; ++j) v[j] = s4[j];          // 4 pixels * BPP bytes = BPP dwords, all inside the row
    } else {
        const int nb = (x1 - x0) * BPP;                      // the bytes of this lane's own pixels, no more
        PIXFMT_TOUCH(0, s, nb);
#pragma unroll
        for (int j = 0; j < 4 * BPP; ++j) if (j < nb) v[j >> 2] |= (uint32_t)s[j] << (8 * (j & 3));
    }
    if (full) {
        const uint32_t o = pixfmt_pixel<FMT>(v, 0, shift) | pixfmt_pixel<FMT>(v, 1, shift) << 8 | pixfmt_pixel<FMT>(v, 2, shift) << 16 | pixfmt_pixel<FMT>(v, 3, shift) << 24;
        PIXFMT_TOUCH(1, dst_row + x0, 4);
        *reinterpret_cast<uint32_t*>(dst_row + x0) = o;
    } else {
        PIXFMT_TOUCH(1, dst_row + x0, x1 - x0);
#pragma unroll
        for (int i = 0; i < 3; ++i) if (i < x1 - x0) dst_row[x0 + i] = (uint8_t)pixfmt_pixel<FMT>(v, i, shift);
    }
}

// the same lane with the format chosen at run time (the host harness; the kernel is instantiated per format)
__host__ __device__ inline void pixfmt_lane_any(int format, const uint8_t* src_row, uint8_t* dst_row, int w, int shift, int k)
{
    switch (format) {
    case LVK_PIX_MONO8:  pixfmt_lane<LVK_PIX_MONO8>(src_row, dst_row, w, shift, k); break;
    case LVK_PIX_BGR8:   pixfmt_lane<LVK_PIX_BGR8>(src_row, dst_row, w, shift, k); break;
    case LVK_PIX_RGB8:   pixfmt_lane<LVK_PIX_RGB8>(src_row, dst_row, w, shift, k); break;
    case LVK_PIX_BGRA8:  pixfmt_lane<LVK_PIX_BGRA8>(src_row, dst_row, w, shift, k); break;
    case LVK_PIX_RGBA8:  pixfmt_lane<LVK_PIX_RGBA8>(src_row, dst_row, w, shift, k); break;
    case LVK_PIX_MONO16: pixfmt_lane<LVK_PIX_MONO16>(src_row, dst_row, w, shift, k); break;
    case LVK_PIX_YUYV:   pixfmt_lane<LVK_PIX_YUYV>(src_row, dst_row, w, shift, k); break;
    case LVK_PIX_UYVY:   pixfmt_lane<LVK_PIX_UYVY>(src_row, dst_row, w, shift, k); break;
    default: break;
    }
}
