// What the host-side weight packers (pack.cpp) and the launchers in the kernel files must agree on.  Plain host C++ (no HIP): pack.cpp is compiled without an offload arch.
#pragma once
#include "cer_mvs.h"

// fp32 and f16x3 update-block convs (gru.hip, gru_f16x3.hip): channels a source occupies in the padded K dimension - whole 32-channel chunks
// (CV_KC, HX_KC); the generated disparity source (kind 1, 49 channels): 64
constexpr int PACK_KC = 32;
inline int padded_channels(int ch, int kind) { return kind == 1 ? 64 : ((ch + PACK_KC - 1) / PACK_KC) * PACK_KC; }

// s16 convs (conv_s16.hip): tensors first, the disparity source last; returns the number of disparity sources
inline int sx_order(const int* kind, int nsrc, int* order) {
    int n = 0, nd = 0;
    for (int s = 0; s < nsrc; ++s) if (kind[s] != 1) order[n++] = s;
    for (int s = 0; s < nsrc; ++s) if (kind[s] == 1) { order[n++] = s; ++nd; }
    return nd;
}

// s16 stem (enc_stem.hip): k16-steps of the 7 x 7 x 3 kernel - 7 rows x 2 groups of four columns (4 channel slots each: column 7 and channel 3
// are padding)
constexpr int SM_STEPS = 14;
