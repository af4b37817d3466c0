// The kernel-selection switches (dsg_set_tuning: a test / A-B hook, include/dsg.h): ONE table.  An entry is
//   X(key, field, default, accepted values of `v`)  /* what the switch chooses; what was measured */
// and generates the field of `Tuning` the launch rules read (g_tune.<field>, a plain int), the case of dsg_set_tuning /
// dsg_get_tuning and the name dsg_tuning_key answers to (tuning.hip).  Keep it sorted by key; the header's comment lists the
// same keys and defaults, and tests/test_tuning_cpu.py holds the two against each other.
#pragma once

#define DSG_TUNING_ONOFF (v == 0 || v == 1)
#define DSG_TUNING_LIST(X)                                                                                                      \
  X(1, conv_kc, 0, v == 0 || v == 4 || v == 8)    /* K-chunk of the 3x3 stride-1 f32 MFMA kernel: 4 | 8 | 0 = by grid size (measured, r01) */ \
  X(2, enabled, 1, DSG_TUNING_ONOFF)              /* the fp16x2-split conv kernels (conv_h2*.hip) at all */                       \
  X(3, rows, 0, v == 0 || v == 2 || v == 3 || v == 4) /* rows per wave: 0 = by grid size, 2 | 4 forced, 3 = by grid size but no 16-row tiles below 256 workgroups */ \
  X(5, stats, 1, DSG_TUNING_ONOFF)                /* epilogue GroupNorm statistics (A/B against the separate pass) */             \
  X(6, waves, 4, v == 4 || v == 8)                /* 16-row tiles: 4 waves x 4 rows or 8 waves x 2 rows */                        \
  X(7, wgrad_h2, 1, DSG_TUNING_ONOFF)             /* 3x3 / pointwise weight gradients on the split path (A/B against the f32 MFMA) */ \
  X(8, fold, 1, DSG_TUNING_ONOFF)                 /* folded up-sampler convs (A/B against the x2 gather) */                       \
  X(10, conv_fewout, 1, DSG_TUNING_ONOFF)         /* VALU kernel for cout <= 4 (A/B against the zero-padded MFMA tile) */         \
  X(11, pw_occ2, 1, DSG_TUNING_ONOFF)             /* pointwise convs: 8-row tiles compiled for two workgroups per CU */           \
  X(13, unet_blocked, 1, DSG_TUNING_ONOFF)        /* intermediates of dsg_unet_forward in the channel-blocked layout (A/B against [N,C,H,W]) */ \
  X(14, att_mfma, 1, DSG_TUNING_ONOFF)            /* attention with head_dim 8 on the matrix cores (A/B against the VALU kernel) */ \
  X(15, s2, 1, DSG_TUNING_ONOFF)                  /* stride-2 convs on the split path (A/B against the f32 MFMA kernel) */        \
  X(16, bm32, 0, v >= 0)                          /* 32-cout x 8-row workgroups, two per CU, for the shallow levels: 0 | 1 | n > 1 = when the 64-cout x 16-row grid has at least n workgroups, see bm32_min() (measured slower than the 64 x 16 geometry: 0.356 vs 0.302 ms at 64 channels / 256^2 -- off) */ \
  X(17, bm32_small, 1, DSG_TUNING_ONOFF)          /* 32-cout workgroups for grids of at most half the CUs */                      \
  X(18, bm128, 1, DSG_TUNING_ONOFF)               /* 16-bit modes: 128-cout workgroups where the grid still fills the chip */     \
  X(19, splitk, 1, DSG_TUNING_ONOFF)              /* split-K for grids of at most half the CUs, when the caller gives scratch */  \
  X(20, ws2, 1, DSG_TUNING_ONOFF)                 /* fp32-equivalent 3x3 convs with cin <= 128: 8-row tiles, one weight slab, two workgroups per CU */ \
  X(21, conv_in, 1, DSG_TUNING_ONOFF)             /* conv_in.hip's own kernel (its switch moves the plan's statistics buffers too) */ \
  X(22, conv_out, 1, DSG_TUNING_ONOFF)            /* conv_out.hip's own kernel */                                                 \
  X(23, fuse_sc, 1, DSG_TUNING_ONOFF)             /* resnet shortcuts fused into conv2's K loop (A/B against the separate 1x1 kernel) */ \
  X(25, att_blocked, 1, DSG_TUNING_ONOFF)         /* the plan keeps q, k, v and the attention output channel-blocked (the plan's arena changes with it) */ \
  X(26, pre, 1, DSG_TUNING_ONOFF)                 /* pre-staged operand images for the layers with >= pre_min_ct cout tiles per patch */ \
  X(27, pre_min_ct, 16, v >= 1)                   /* ... the threshold.  Measured, profiles/r03_operand_ablation.txt: at 4 -- every conv of the 256- / 512-channel levels -- the convs gain 8.5 % and the prepare passes cost what they gain; at 16 only the folded up-samplers of those levels qualify, whose patch is staged by 16-32 workgroups */ \
  X(29, wgrad16_wide, 1, DSG_TUNING_ONOFF)        /* 16-bit 3x3 weight gradients: 0 = the 64 x 64 workgroup everywhere */         \
  X(30, wgrad16_pw, 1, DSG_TUNING_ONOFF)          /* 16-bit pointwise weight gradients: 0 = the 3x3 kernel's one-tap instantiation */ \
  X(31, wgrad_h2_wide, 1, DSG_TUNING_ONOFF)       /* fp32-equivalent 3x3 weight gradients: 0 = the 32 x 64 workgroup everywhere */ \
  X(32, narrow, 1, DSG_TUNING_ONOFF)              /* maps narrower than a tile (16 x 16, 8 x 8) also take split-K, the folded up-sampler and the stride-2 kernel (0 = one-slice plain kernel / exact f32 MFMA kernels for them, the rule before round 4) */ \
  X(34, splitk_mid, 1, DSG_TUNING_ONOFF)          /* split-K also for grids of 129 .. 170 workgroups with K >= 24 chunks: 3 slices */ \
  X(36, rows_rule, 1, DSG_TUNING_ONOFF)           /* round 5's additions to the rows rule: 16-row tiles under three-slice split-K, 0.62 for the four-tap kernels */ \
  X(37, gnb, 1, v >= 0 && v <= 3)                 /* GroupNorm-backward statistics from the data-gradient conv's epilogue (A/B against the statistics pass): 0 | 1 | 2 | 3, see gnb_mode() / gnb_seam64() */ \
  X(38, att_bwd_split, 1, DSG_TUNING_ONOFF)       /* the fp32 tape's attention backward on the matrix cores, fp16x2 split (A/B against the VALU kernels) */ \
  X(39, wgrad16_fold, 1, DSG_TUNING_ONOFF)        /* 16-bit weight gradient of Upsample2D's conv folded: 0 = the nine-tap kernel at full resolution */ \
  X(40, s2_nchw, 1, DSG_TUNING_ONOFF)             /* stride-2 convs of fp32 [N,C,H,W] tensors on the space-to-depth kernel too (A/B against the exact f32 kernel) */ \
  X(41, gnb_bm64, 1, DSG_TUNING_ONOFF)            /* 16-bit data-gradient convs with the GNB epilogue on 64-cout workgroups, two per CU (0 = 128-cout ones where the plain conv takes them) */

namespace dsg {

struct Tuning {
#define DSG_TUNING_FIELD(key, field, dflt, ok) int field = dflt;
  DSG_TUNING_LIST(DSG_TUNING_FIELD)
#undef DSG_TUNING_FIELD
  int epoch = 0;  // bumped by every accepted dsg_set_tuning call: host-side caches of kernel-selection answers key on it
  // the two keys whose value says more than one thing (the fields above hold the value as given)
  int gnb_mode() const { return gnb == 3 ? 1 : gnb; }   // 0 off | 1 every GNB kernel | 2 only the two-per-CU 64-cout ones
  bool gnb_seam64() const { return gnb != 3; }          // ... also where the two x tensors meet inside a channel tile, at a multiple of 32 channels
  bool bm32_on() const { return bm32 != 0; }
  int bm32_min() const { return bm32 > 1 ? bm32 : 512; }  // ... when the 64-cout x 16-row grid has at least this many workgroups
};
extern Tuning g_tune;  // tuning.hip

}  // namespace dsg
