// rx_internal.h -- the library's internal interface: every function without C linkage that one .hip file defines and another
// calls.  The defining file and the calling files include this header, so a changed signature fails to compile.
#pragma once
#include "rx_common.h"

// ---- rx_runtime.hip
int rx_note_seq(void);   // how many times rx_note_kernel ran on this thread

// ---- rx_conv_halo.hip, rx_pointwise.hip, rx_dgrad_s2.hip: the fast paths of the conv entry points in rx_igemm.hip.  Which of them
// a call takes is decided by the routes of rx_gather_plan.h (the halo kernels: rx_ch_choose, rx_conv_halo_plan.h); these launch
// the choice they are handed and return RX_OK or an error.
// rx_conv_halo_launch, stat_part / bs: a choice with take_stats leaves per-wave partial rows in stat_part, c.stat_chunks per sample
// -- forward the sums of y and y^2, backward-data with take_bs the two InstanceNorm backward sums of the layer `bs` describes.
int rx_conv_halo_launch(const RxChChoice& c, rx_dtype dt, const rx_act* in, const void* w, const float* bias, const rx_act* out, int flip,
                        int accumulate, hipStream_t st, float* stat_part, const RxBwdStat* bs);
int rx_pointwise_launch(const RxPwChoice& c, rx_dtype dt, const void* in, const void* w, const float* bias, void* out, hipStream_t st,
                        const char* who);
int rx_dgrad_s2_launch(const RxDs2Choice& c, rx_dtype dt, const void* dy, const void* w_bwd, void* dx, hipStream_t st);

// ---- rx_wgrad_halo.hip: fast path of rx_conv3d_bwd_weight (rx_wgrad.hip), chosen by rx_wgh_choose (rx_wgrad_plan.h)
int rx_wgrad_halo_launch(const RxWghChoice& c, rx_dtype dt, const void* x, const void* dy, float* dw, void* ws, hipStream_t st);
// ---- rx_wgrad.hip: the split reduce both weight-gradient files end with
void rx_wgrad_reduce_launch(const float* slab, int S, int T_, int R, int C, float* dw, hipStream_t st);

// ---- rx_stem_wgrad.hip: MFMA variants of the stem kernels, tried first by the entry points in rx_stem.hip
int rx_stem_fwd_mfma_try(rx_dtype dt, const float* x, int n, int cin, int z, int y, int xx, const float* w, const float* bias,
                         const rx_act* out, const int32_t kernel[3], hipStream_t st, float* stat_part, size_t stat_bytes, int* stat_chunks);
int rx_stem_wgrad_mfma_try(rx_dtype dt, const float* x, int n, int cin, int z, int y, int xx, const rx_act* dy, const int32_t kernel[3],
                           float* partial, int max_blocks, int* nblocks_out, hipStream_t st);

// ---- rx_instnorm.hip: finalize launches over per-chunk partials laid out like colreduce_kernel's (rx_reduce.h)
// `mode` is one of the FIN_* modes of rx_reduce.h
void rx_colreduce_finalize_launch(hipStream_t st, const float* partial, int N, int nchunks, int nacc, int C, double V, float eps, int mode,
                                  float* out);
void rx_stats_finalize_launch(const float* partial, int N, int nchunks, int C, double V, float eps, float* stats, hipStream_t st);
void rx_inbwd_fused_finalize_launch(const float* partial, int N, int nchunks, int C, double V, const float* stats, float* m12, hipStream_t st);
