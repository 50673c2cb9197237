// maskmlp.h - the geometry of MaskField (3 -> 128 x 4 ReLU -> K <= 32, softmax) on the fp32 MFMA sample-tile engine that mask.hip
// (nvfi_maskfield_fwd / _bwd on free points) and maskloss.hip (the same MLP over a render's masked list) must agree on: the stash rows of a
// tile, the fragment sizes and their order in a workspace, the slab room of the five weight-gradient jobs.  One copy: a change here moves both.
#pragma once
#include "engine.h"

#define MK_F_ROWS (16 + 4 * 64 + 16)   // forward stash per tile: x0 (16) | h1..h4 (64 each) | softmax (16)
#define MK_B_ROWS (16 + 4 * 64)        // backward stash per tile: g_logits (16) | g_z4, g_z3, g_z2, g_z1 (64 each)
#define MK_NSLAB 256
#define MK_SLAB_FLOATS (128 * 128 + 128)
#define MK_F0 (4 * 2 * 64)
#define MK_FH (4 * 64 * 64)
#define MK_F4 (1 * 64 * 64)
#define MK_T4 (4 * 16 * 64)            // transposed last layer: rows = 128 hidden features, slots = 32 logit rows
#define MK_FRAG_FLOATS (MK_F0 + 3 * MK_FH + MK_F4 + 5 * 128 + MK_T4 + 3 * MK_FH)
#define MK_MASK_WORDS (4 * 128)        // ReLU sign words per tile: [hidden layer 0..3][lo | hi][64 lanes]

struct MkFrags { const float* f[5]; const float* b[5]; const float* t[5]; };   // t[0] unused (no gradient wrt the points)

// fragment pointers inside a workspace region of MK_FRAG_FLOATS floats: forward fragment + 128 bias floats per layer, then the four transposed
// (dgrad) fragments of layers 1..4 - the order mask_frags (mask.hip) packs and every reader walks
static inline void mk_frag_ptrs(float* frag, MkFrags* W) {
    float* p = frag;
    for (int l = 0; l < 5; ++l) { const int MT = l < 4 ? 4 : 1, NS = l == 0 ? 2 : 64; W->f[l] = p; p += MT * NS * 64; W->b[l] = p; p += 128; }
    W->t[0] = nullptr;
    for (int l = 1; l < 5; ++l) { const int NS = l < 4 ? 64 : 16; W->t[l] = p; p += 4 * NS * 64; }
}
