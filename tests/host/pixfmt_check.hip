// tests/host/pixfmt_check.hip — stand-alone host harness of larvio_amd/csrc/fe_pixfmt_dev.h, built with
//   hipcc -Xarch_host -fsanitize=address,undefined  and run by tests/test_pixfmt_ref.py (no GPU, no Python in the process).
// It drives pixfmt_lane exactly as k_image_to_gray does - every lane index the launch would cover for a row, the padding lanes of the
// last block included - on rows that own their memory: a source row of w * bytes_per_pixel bytes ends where its heap block ends, and
// starts where the block starts (offset 0) or 1..3 bytes in; the destination row likewise.  A byte read or written past the end of a
// row is an AddressSanitizer report.  In FRONT of a row that starts 1..3 bytes into its block the sanitizer cannot look (its shadow
// marks whole 8-byte granules from their first byte), so the header's PIXFMT_TOUCH hook records every range a lane loads or stores and
// the harness holds the union to the row.  Results are compared with the plain loop below, written from the text of include/lvk_c.h.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

static const uint8_t *g_lo[2], *g_hi[2];
static long g_vec_lanes = 0;
#define PIXFMT_TOUCH(kind, ptr, nbytes)                                                   \
    do {                                                                                  \
        const uint8_t* p_ = (const uint8_t*)(ptr);                                        \
        if (!g_lo[kind] || p_ < g_lo[kind]) g_lo[kind] = p_;                              \
        if (!g_hi[kind] || p_ + (nbytes) > g_hi[kind]) g_hi[kind] = p_ + (nbytes);        \
        if ((kind) == 0 && (nbytes) >= 4 && ((uintptr_t)p_ & 3u) == 0 && (nbytes) % 4 == 0) ++g_vec_lanes; \
    } while (0)
#include "fe_pixfmt_dev.h"

static unsigned plain_pixel(int format, const uint8_t* px, int shift)
{
    switch (format) {
    case LVK_PIX_MONO8: return px[0];
    case LVK_PIX_BGR8: case LVK_PIX_BGRA8: return (1868u * px[0] + 9617u * px[1] + 4899u * px[2] + 8192u) >> 14;
    case LVK_PIX_RGB8: case LVK_PIX_RGBA8: return (1868u * px[2] + 9617u * px[1] + 4899u * px[0] + 8192u) >> 14;
    case LVK_PIX_MONO16: { uint16_t v; memcpy(&v, px, 2); const unsigned s = (unsigned)v >> shift; return s > 255u ? 255u : s; }
    case LVK_PIX_YUYV: return px[0];
    default: return px[1];
    }
}

int main()
{
    static const int widths[] = {1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64, 65};
    unsigned seed = 12345u;
    long rows = 0, bad = 0;
    for (int format = 0; format < 8; ++format) {
        const int bpp = lvk_pixfmt_bpp(format);
        for (int wi = 0; wi < (int)(sizeof widths / sizeof widths[0]); ++wi) {
            const int w = widths[wi];
            if ((format == LVK_PIX_YUYV || format == LVK_PIX_UYVY) && (w & 1)) continue;
            for (int so = 0; so < 4; ++so) {
                if (format == LVK_PIX_MONO16 && (so & 1)) continue;          // the entry refuses an odd mono16 address
                for (int d_o = 0; d_o < 4; ++d_o) {
                    const int shift = format == LVK_PIX_MONO16 ? (int)(rows % 9) : 0;
                    const size_t nb = (size_t)w * bpp;
                    uint8_t* sblock = (uint8_t*)malloc(so + nb); uint8_t* dblock = (uint8_t*)malloc(d_o + (size_t)w);
                    uint8_t* src = sblock + so; uint8_t* dst = dblock + d_o;
                    if (((uintptr_t)sblock & 15u) || ((uintptr_t)dblock & 15u)) { printf("malloc alignment\n"); return 2; }
                    for (size_t i = 0; i < so + nb; ++i) { seed = seed * 1664525u + 1013904223u; sblock[i] = (uint8_t)(seed >> 24); }
                    memset(dblock, 0xA5, d_o + (size_t)w);
                    g_lo[0] = g_hi[0] = g_lo[1] = g_hi[1] = nullptr;
                    // the launch: blocks of 256 lanes over the widest row ((w + 3 + 3) / 4 lanes), every lane of every block
                    const int blocks = ((w + 6) / 4 + 255) / 256;
                    for (int k = blocks * 256 - 1; k >= 0; --k) pixfmt_lane_any(format, src, dst, w, shift, k);       // any order: lanes are independent
                    if (pixfmt_row_lanes(dst, w) > blocks * 256) { printf("launch too small\n"); return 2; }
                    for (int x = 0; x < w; ++x)
                        if (dst[x] != plain_pixel(format, src + (size_t)x * bpp, shift)) {
                            if (++bad < 10) printf("mismatch: format %d w %d src+%d dst+%d x %d: %u, want %u\n", format, w, so, d_o, x, dst[x], plain_pixel(format, src + (size_t)x * bpp, shift));
                        }
                    for (int i = 0; i < d_o; ++i) if (dblock[i] != 0xA5) { ++bad; printf("byte in front of the destination row written: format %d w %d\n", format, w); }
                    if (g_lo[0] != src || g_hi[0] != src + nb) { ++bad; printf("loads cover [%ld, %ld) of a %zu-byte row: format %d w %d src+%d dst+%d\n", (long)(g_lo[0] - src), (long)(g_hi[0] - src), nb, format, w, so, d_o); }
                    if (g_lo[1] != dst || g_hi[1] != dst + w) { ++bad; printf("stores cover [%ld, %ld) of a %d-byte row: format %d w %d src+%d dst+%d\n", (long)(g_lo[1] - dst), (long)(g_hi[1] - dst), w, format, w, so, d_o); }
                    free(sblock); free(dblock);
                    ++rows;
                }
            }
        }
    }
    printf("pixfmt_check: %ld rows, %ld vectorised lanes, %ld mismatches\n", rows, g_vec_lanes, bad);
    return bad ? 1 : 0;
}
