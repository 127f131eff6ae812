/* libpggan_hip.so — diagnostic exports (NOT part of the drop-in boundary).
 *
 * Tuning and attribution aids used by bench.py and tools/: they read / set THREAD-LOCAL state of the calling thread
 * (the last launched kernel symbol, a forced tile configuration), which the product path never touches.  Kept apart
 * from pggan_hip.h so that the product header states its re-entrancy contract without exceptions. */
#ifndef PGGAN_HIP_DEBUG_H
#define PGGAN_HIP_DEBUG_H

#ifdef __cplusplus
extern "C" {
#endif

/* Profiling aid: symbol (as rocprofv3 prints it, e.g. "conv_igemm_kernel<3, 4, 2, 2, 4>") of the kernel instantiation most
 * recently launched by the calling thread through pg_conv2d_*_nhwc / pg_conv2d_wgrad_*_nhwc, pg_conv2d_wino_nhwc,
 * pg_conv2d_wgrad_wino_nhwc ("" before the first launch): lets bench.py attribute its HIP-event timings to the exact
 * symbol that rocprofv3 --kernel-trace --stats reports. */
const char* pg_debug_last_conv_kernel(void);
const char* pg_debug_last_wino_kernel(void);
const char* pg_debug_last_wino_wgrad_kernel(void);

/* Tuning aids (tools/sweeps/): force a configuration of the direct conv / weight-gradient kernels (csrc/conv_igemm.hip, conv_thin.hip,
 * conv_k4.hip, conv_wgrad.hip; the switches themselves live in conv_api.hip) for the calling thread's next launches.  Value -1 restores the built-in choice of a key.  Callers pass the integers. */
enum pg_tune_key {
    PG_TUNE_CONV_TILE = 0,      /* value: index of the tile candidate (conv_igemm.hip, dispatch_conv) */
    PG_TUNE_WGRAD = 1,          /* value: enum pg_wgrad_cfg */
    PG_TUNE_SPLITK = 2,         /* value: K slices of a conv / workgroup chunks of a weight gradient (1: never split) */
    PG_TUNE_PATH = 3            /* value: enum pg_path */
};
enum pg_wgrad_cfg {             /* 0 (any other value >= 0): the 32 x 16 block with 64-pixel tiles, whatever the launch size */
    PG_WGRAD_32x16_128PX = 1,   /* wide 3x3 layers: 32(cout) x 16(cin) block, 128-pixel tiles */
    PG_WGRAD_64x16_64PX = 3,    /* wide 3x3 layers: 64(cout) x 16(cin) block, 64-pixel tiles */
    PG_WGRAD_TILE_NOT_STRIP = 20 /* 8/16-channel layers: the block-MFMA tile kernel instead of the row-streaming one */
};
enum pg_path {
    PG_PATH_NO_THIN = 2,        /* generic tile kernel for the 8/16-cout layers (no block-MFMA / row-streaming kernel) */
    PG_PATH_NO_SMALLMAP_SPLIT = 8, /* never the forced split-K of deep layers on small maps */
    PG_PATH_SMALLMAP_SPLIT_2304 = 9, /* that split up to 2304 output pixels instead of 576 */
    PG_PATH_UNFUSED_PIXELNORM = 11, /* PixelNorm as a second pass instead of the conv's epilogue */
    PG_PATH_NO_THIN_POOL16 = 17, /* 8 -> 16 + pool with sign bytes: generic tile kernel instead of the block-MFMA one */
    PG_PATH_TILE_NOT_STRIP = 20, /* 8-cout layers: the block-MFMA tile kernel instead of the row-streaming one */
    PG_PATH_K4_ONE_WORKGROUP = 21 /* 4x4 -> 1x1 layer: one workgroup per cout block, no slicing through the workspace */
};
int pg_debug_set_tuning(int key, int value);
/* Winograd conv variant: 0 built-in choice; 11 / 12: tile kernel with 16 / 32 couts per workgroup; 20: tile kernels only;
 * 21: the row-streaming kernel wherever it exists, general epilogue included.  Anything else: PG_E_ARG. */
int pg_debug_set_wino(int vec);
/* K slices per (tile block, cout block) of the Winograd tile conv: -1 built-in choice, 0 / 1 never split, n: n slices
 * wherever a scratch is registered (pg_set_workspace) and the layer has that many 8-channel chunks. */
int pg_debug_set_wino_ksplit(int n);
/* 0: the general epilogue for every launch of the Winograd tile conv (A/B against the specialised ones); -1: built-in choice. */
int pg_debug_set_wino_epi(int mode);

#ifdef __cplusplus
}
#endif
#endif /* PGGAN_HIP_DEBUG_H */
