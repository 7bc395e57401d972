// Letter thumbnails (avae_letter_thumbnail; include/avae.h): the definition, the plan, the launch shapes and
// the kernel arguments shared by the host (avae_host.hip) and the kernels (avae_thumbnail.hip).
//
// The definition (every step integer arithmetic; tests/thumbnail_reference.py restates it in NumPy int64):
//   grey   v = the byte (C = 1), or (4899 R + 9617 G + 1868 B + 8192) >> 14 (C = 3, 4; bgr swaps the first and third byte, a
//          fourth byte is ignored)
//   ink    threshold < 0:  g = invert ? 255 - v : v;   else  t = v > threshold ? 255 : 0,  g = invert ? 255 - t : t.
//          g != 0  <=>  (v > T) != invert  with  T = threshold, or without one T = invert ? 254 : 0  (thumb_ink_level)
//   box    (x, y, w, h) the bounding box of the pixels with g != 0, ink their count; no ink: (0, 0, Wf, Hf), ink 0
//   window L = max(w, h), b = 3 L / 5, S = L + b, oy = b / 2 + (L - h) / 2, ox = b / 2 + (L - w) / 2: frame pixel (y + r, x + c) is
//          cell (oy + r, ox + c) of an S x S canvas of zeros;  window = (x - ox, y - oy, S)
//   image  sum(i, j) = sum_rows sum_cols g wy(i, row) wx(j, col),  wx(j, k) = max(0, min((j + 1) S, (k + 1) Ho) - max(j S, k Ho)),
//          wy likewise;  image[i Ho + j] = (float)((double)sum / (double)(255 S S)): one division in double, one rounding
//
// k_ink_box    grid slabs x rows (one dimension, the slab the fast index), 256 threads.  A workgroup scans the frame rows
//              [slab * slab_rows, min(Hf, (slab + 1) * slab_rows)), wave v the rows v, v + 4, ... of them.  The bytes of a row
//              are cut at the 16-byte lines of memory: the whole 16-byte chunks inside the row are loaded as one dwordx4 per
//              lane, consecutive lanes on consecutive chunks, and a lane owns the pixels that START in its chunk (a pixel of
//              3 or 4 bytes may end in the next 4 bytes: one more dword, or, behind the row's last whole chunk, its bytes one
//              by one).  The at most 15 + 15 pixels that start before the first or behind the last whole chunk -- all of them
//              in a row shorter than a chunk -- are loaded byte by byte, a pixel per lane.  No byte outside [row, row + Wf C) is
//              ever loaded.  A lane keeps min / max column, min / max row and the count; the wave reduces them with shuffles, the
//              four waves through LDS, and thread 0 writes the workgroup's record {x0, x1, y0, y1, count, 0, 0, 0} (x1, y1
//              inclusive; no ink: x0 = y0 = INT_MAX, x1 = y1 = -1, count 0).  Every record is written on every call.
// k_thumbnail  grid size x rows (one dimension, the output row the fast index), 256 threads.  Every workgroup merges the
//              frame's records (min, max, sum) and derives the window.  Workgroup i forms output row i: thread t owns the crop
//              columns t, t + 256, ... (at most 16), one after another, and adds wy(i, row) g over the canvas rows [i S / Ho,
//              ceil((i + 1) S / Ho)) that meet the crop, in 32-bit integers (<= 255 S), consecutive lanes on consecutive pixels, the
//              loads of four rows in flight.  The column sums go to LDS.
//              Then min(64, 256 / Ho rounded down to a power of two) threads per output pixel j add wx(j, col) times the column
//              sums of their columns in 64 bits, a shuffle tree joins them, and one thread divides and stores.  A blank frame's
//              row is stored as +0 without a load.  Workgroup 0 of a frame writes box, window and ink.
// The sums are integers, so their order changes no bit.  No atomics, no scratch; the kernels read and write no model state.
// LDS and registers (hipcc -O3, gfx950): DESIGN.md section 30.
#pragma once
#include "avae_latent_common.h"

namespace avae {

constexpr int kThumbThreads = 256;
constexpr int kThumbMaxFrame = 4096, kThumbMaxSize = 64, kThumbMaxSlabs = 64;
constexpr int kThumbMaxRows = 1 << 24;       // rows * 64 workgroups in one grid dimension
constexpr long long kThumbMaxRowStride = 1ll << 26, kThumbMaxFrameStride = 1ll << 38;   // rows * frame_stride stays below 2^63
constexpr int kThumbSlabPixels = 8192;      // a slab is at least this many pixels (or the whole frame)
constexpr int kThumbCols = kThumbMaxFrame / kThumbThreads;   // crop columns per thread of k_thumbnail, at most
static_assert(kThumbCols * kThumbThreads == kThumbMaxFrame, "a thread's columns t, t + 256, ... cover the widest crop");
constexpr int kThumbRecordInts = 8;          // x0, x1, y0, y1, count, three zeros: 32 bytes

struct ThumbPlan { int slab_rows, slabs; };
inline ThumbPlan thumb_plan(int Hf, int Wf) {
    const int by_count = (Hf + kThumbMaxSlabs - 1) / kThumbMaxSlabs, by_size = (kThumbSlabPixels + Wf - 1) / Wf;
    const int slabs = (Hf + std::max(by_count, by_size) - 1) / std::max(by_count, by_size);
    return {(Hf + slabs - 1) / slabs, slabs};     // slab s covers the rows [s * ceil(Hf / slabs), ...): none is empty
}
inline size_t thumb_workspace_bytes(long long rows, int slabs) { return (size_t)rows * slabs * kThumbRecordInts * sizeof(int32_t); }

// g != 0  <=>  (v > level) != invert
__host__ __device__ inline int thumb_ink_level(int threshold, bool invert) { return threshold >= 0 ? threshold : invert ? 254 : 0; }

struct ThumbArgs {
    const uint8_t* frames;        // [rows][Hf][Wf][C] with the two strides below
    long long row_stride, frame_stride;   // bytes
    int32_t* records;             // [rows][slabs][kThumbRecordInts]
    float* image;                 // [rows][size * size] or NULL
    int32_t* box;                 // [rows][4] or NULL
    int32_t* window;              // [rows][3] or NULL
    int32_t* ink;                 // [rows] or NULL
    int Hf, Wf, C;
    int invert, bgr, threshold;   // threshold < 0: none
    int size, slab_rows, slabs;
};

void launch_ink_box(const ThumbArgs& a, long long rows, hipStream_t s);
void launch_thumbnail(const ThumbArgs& a, long long rows, hipStream_t s);

}  // namespace avae
