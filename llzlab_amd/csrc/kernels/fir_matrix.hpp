// fir_matrix.hpp -- what fir_matrix.hip (K4g) and fir_matrix_fade.hip (K4g while paths fade) share beyond stream_bins.hpp: the
// geometry of a launch, the product's bins per thread and tiles per block, and the shape check of the entries.  No device code
// lives here: the kernels of the two files are written out side by side, the inverse included, whose fold into one function
// of this header was built, measured and taken out again ("Shared code").
#pragma once
#include "stream_bins.hpp"

namespace {

struct matrix_geom {
    int inputs, outputs, P, R, head;
    int nblk;                   // blocks of this launch
    int flush, j0;              // a flush in several passes: the block of the flush that is block 0 of this launch
    int G, gsize;               // input groups, inputs per group (the last group may hold fewer)
    long n_out;                 // samples per output to store: <= nblk B
    long in_pitch, out_pitch;
};

// bins per thread and per workgroup of the product
constexpr int mac_v(int log2b) { return log2b >= 9 ? 2 : 1; }
constexpr int mac_tiles(int log2b) { return (1 << log2b) / (stream_threads(log2b) * mac_v(log2b)); }

constexpr unsigned GRID_YZ_MAX = 65535u;

// what the entries share: the shape within the kernels' index ranges and the grid limits
bool matrix_shape_ok(int log2ok, int inputs, int outputs, int nblk, int P, int R, int head)
{
    return log2ok && inputs >= 1 && inputs <= 4096 && outputs >= 1 && outputs <= 4096 && nblk >= 1 &&
           (unsigned)nblk <= GRID_YZ_MAX && P >= 1 && R >= P && head >= 0 && head < R;
}

// the product's group arguments within the grid's z limit, and a flush pass within the partitions
bool matrix_groups_ok(int block, int inputs, int nblk, int flush, int j0, int P, int groups, int group_size)
{
    return groups >= 1 && group_size >= 1 && (long)groups * group_size >= inputs && (long)(groups - 1) * group_size < inputs &&
           (unsigned)groups * (unsigned)(block / 64) <= GRID_YZ_MAX && j0 >= 0 && (flush || j0 == 0) &&
           (!flush || (long)j0 + nblk <= P);
}

} // namespace
