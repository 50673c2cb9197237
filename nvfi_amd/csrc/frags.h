// frags.h - the packed weight images of a field: the persistent fragment cache (round 5, ABI v5: nvfi_field_desc.frags) and the ONE way a
// host entry point gets the velocity net's images (vel_images).  Which images a warp needs, and which kernel it launches, is warp.h's.
//
// The MFMA kernels read the Linear weights in fragment order (engine.h).  Rounds 1-4 repacked them inside every call into the call's
// workspace - 3 k_pack + 4 k_frag_x4 launches per training iteration for weights that change once per iteration.  nvfi_pack_frags writes
// EVERY fragment set the render and PDE calls use - render MLP + basis_mat (forward, transposed), both velocity nets (forward, transposed,
// biases) and the x4 copies of the feature-split kernels - into one caller-owned buffer in ONE launch; a call whose descriptor carries the
// buffer (nvfi_field_desc.frags != NULL) skips its pack launches and reads the fragments from it.  The caller repacks after every change of
// the weights (the Python mirror keys the buffer on the parameters' versions).
#pragma once
#include "common.h"
#include "pde.h"
#include "x6.h"

// ---------------------------------------------------------------- the velocity net's images
// VI_VEL / VI_ANET: the plain MFMA fragments (VelFrags) of weight_net / a_weight_net; VI_X4F / VI_X4B: x4 copies of weight_net's forward /
// transposed fragments; VI_A_X4B: of a_weight_net's transposed fragments; VI_X6 / VI_X6T: the three-term bfloat16 image of weight_net / its transpose
enum { VI_VEL = 1, VI_ANET = 2, VI_X4F = 4, VI_X4B = 8, VI_A_X4B = 16, VI_X6 = 32, VI_X6T = 64 };
struct VelImageRoom { float *vel, *anet, *x4f, *x4b, *a_x4b; void *x6, *x6t; };     // the call's own workspace, NULL where its plan has none
struct VelImages { VelFrags VW, AW; const float4 *f4[6], *t4[6], *ta4[6]; const void *x6, *x6t; };
// The images `need` names, and nothing else, in *out.  With f->frags they are the cache's and nothing is launched.  Without, they are packed into
// `room` with the per-call pack kernels - one k_pack for the plain fragments, one k_frag_x4 for weight_net's x4 copies, one for a_weight_net's,
// one x6 pack - except those `have` names: the room holds them already (the render backward behind its forward).  An image that is needed, not
// cached and has no room is error 3 naming it.  ride: plain pack jobs of the caller (the render MLP's) that share the k_pack launch of an
// uncached call, or NULL; a cached call's are dropped, as its fragments are the cache's too (render_frag_room).
int vel_images(const nvfi_field_desc* f, unsigned need, const VelImageRoom& room, VelImages* out, const PackJobs* ride, unsigned have, hipStream_t st);
// where the render MLP's fragments of a call live: the cache's region, or the call's own room
float* render_frag_room(const nvfi_field_desc* f, float* own);

int launch_pack_all(const PackJobsAll& jobs, const X6PackArgs* x6, hipStream_t st);
