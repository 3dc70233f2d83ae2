// The median cut of the GIF writer (REFace/scripts/VFace_inference_batch.py:658), written once for the device and the host:
// csrc/gif.hip calls these routines between its scans over the 32768 cells, tests/gif_probe.cpp calls them from a plain C++ program
// under the address and undefined-behaviour sanitizers, and tests/gif_model.py restates them in Python.
//
// A frame's colours are counted in cells of 8 x 8 x 8: cell(r, g, b) = (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3).  Box 0 holds every
// non-empty cell.  Up to 255 times one box is split in two; every choice is an integer rule made HERE:
//   1. which box: one with at least two non-empty cells and the largest population x longest side in cells; the lowest box number
//      on a tie (vf_gif_box_key: the comparison of one 64-bit key);
//   2. which axis: the longest side, ties in R, G, B order (vf_gif_box_axis);
//   3. where: with m[v] the box's population at coordinate v of that axis, the smallest v with 2 (m[lo] + .. + m[v]) >= population,
//      but at most hi - 1, so that both sides keep a non-empty cell (vf_gif_box_cut).  Cells above the cut take the next free box number.
// vf_gif_boxes_serial is the whole cut on one thread: the host's way through the same three routines.
// This file has no include of the HIP runtime: a C++17 host compiler reads it as it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VF_GIF_HD __host__ __device__ inline
#else
#define VF_GIF_HD inline
#endif

constexpr int kGifCells = 32768;
constexpr int kGifColors = 256;

struct VfGifBox {
    uint32_t pop;            // pixels
    int32_t ncells;          // non-empty cells
    int32_t lo[3], hi[3];    // of the non-empty cells, in cells, R G B
};

VF_GIF_HD int vf_gif_cell(int r, int g, int b) { return (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3); }
VF_GIF_HD int vf_gif_cell_coord(int cell, int axis) { return (cell >> (10 - 5 * axis)) & 31; }

// 0 for a box that cannot be split; otherwise the box with the largest key is split next.  pop <= 2^24 (the histogram's bound), a
// side <= 32: the product stays below 2^30.
VF_GIF_HD uint64_t vf_gif_box_key(const VfGifBox& b, int i) {
    if (b.ncells < 2) return 0;
    int side = b.hi[0] - b.lo[0];
    if (b.hi[1] - b.lo[1] > side) side = b.hi[1] - b.lo[1];
    if (b.hi[2] - b.lo[2] > side) side = b.hi[2] - b.lo[2];
    return ((uint64_t)b.pop * (uint64_t)(side + 1)) << 8 | (uint64_t)(255 - i);
}

VF_GIF_HD int vf_gif_box_axis(const VfGifBox& b) {
    const int r = b.hi[0] - b.lo[0], g = b.hi[1] - b.lo[1], bl = b.hi[2] - b.lo[2];
    return (r >= g && r >= bl) ? 0 : (g >= bl ? 1 : 2);
}

// marg[32]: the population at every coordinate of the axis -> the last coordinate of the lower side; lo < hi
VF_GIF_HD int vf_gif_box_cut(const uint32_t* marg, int lo, int hi, uint32_t pop) {
    uint64_t run = 0;
    int v = lo;
    for (; v < hi; ++v) {
        run += marg[v];
        if (2 * run >= pop) break;
    }
    return v < hi - 1 ? v : hi - 1;
}

VF_GIF_HD void vf_gif_box_reset(VfGifBox& b) {
    b.pop = 0; b.ncells = 0;
    for (int a = 0; a < 3; ++a) { b.lo[a] = 31; b.hi[a] = 0; }
}

VF_GIF_HD void vf_gif_box_add(VfGifBox& b, int cell, uint32_t count) {
    b.pop += count; ++b.ncells;
    for (int a = 0; a < 3; ++a) {
        const int c = vf_gif_cell_coord(cell, a);
        if (c < b.lo[a]) b.lo[a] = c;
        if (c > b.hi[a]) b.hi[a] = c;
    }
}

// counts [32768] -> labels [32768] (0 for an empty cell), boxes [256]; returns ncolors
VF_GIF_HD int vf_gif_boxes_serial(const uint32_t* counts, uint8_t* labels, VfGifBox* boxes) {
    vf_gif_box_reset(boxes[0]);
    for (int c = 0; c < kGifCells; ++c) {
        labels[c] = 0;
        if (counts[c]) vf_gif_box_add(boxes[0], c, counts[c]);
    }
    int nb = 1;
    while (nb < kGifColors) {
        uint64_t best = 0;
        for (int i = 0; i < nb; ++i) {
            const uint64_t k = vf_gif_box_key(boxes[i], i);
            if (k > best) best = k;
        }
        if (best == 0) break;
        const int i = 255 - (int)(best & 255);
        const int axis = vf_gif_box_axis(boxes[i]);
        uint32_t marg[32];
        for (int v = 0; v < 32; ++v) marg[v] = 0;
        for (int c = 0; c < kGifCells; ++c)
            if (counts[c] && labels[c] == i) marg[vf_gif_cell_coord(c, axis)] += counts[c];
        const int cut = vf_gif_box_cut(marg, boxes[i].lo[axis], boxes[i].hi[axis], boxes[i].pop);
        vf_gif_box_reset(boxes[i]);
        vf_gif_box_reset(boxes[nb]);
        for (int c = 0; c < kGifCells; ++c)
            if (counts[c] && labels[c] == i) {
                const bool upper = vf_gif_cell_coord(c, axis) > cut;
                if (upper) labels[c] = (uint8_t)nb;
                vf_gif_box_add(boxes[upper ? nb : i], c, counts[c]);
            }
        ++nb;
    }
    return nb;
}

// a palette channel: the mean of n >= 1 pixels, halves up
VF_GIF_HD uint32_t vf_gif_mean(uint32_t sum, uint32_t n) { return (uint32_t)((2 * (uint64_t)sum + n) / (2 * (uint64_t)n)); }
