// grm.h -- what grm.hip shares with pca.hip: the kinship accumulator of a call and its finish into a full symmetric matrix.
#pragma once
#include "common.h"

namespace mih {

constexpr int kGrmTile = 128;              // the accumulator tile of one workgroup: four waves, 64 x 64 each

// What the entry points share: the checks, the memory rule, and the accumulator of the kept columns.
struct GrmRun {
    int64_t n = 0, n_pad = 0, m = 0;
    double div = 0.0;
    DevBuf<double> acc, panel;
    DevBuf<int64_t> cols;
};

MIH_LOCAL int launch_failed(const char *what);
// extra_bytes: what the caller's finish will allocate on top (the pair lists, the iteration's blocks); have_out: the caller's
// result pointers are there (looked at after the memory rule, so that a caller who could not allocate an n x n result learns
// what the device lacks)
MIH_LOCAL int grm_accumulate(const char *who, const mih_mat *h, const uint8_t *col_keep, int method, int64_t panel_cols, double extra_bytes,
                             bool have_out, GrmRun &g);
// k_grm_mirror on the stream: g.acc becomes Phi, the n_pad x n_pad symmetric matrix, divided
MIH_LOCAL int grm_mirror(GrmRun &g, hipStream_t s);

}  // namespace mih
