"""The ledger of the convolution family's dispatch branches: one row per (entry point, branch), with the kernel rx_last_conv_kernel()
must report, the dtypes in which the branch exists, the smallest shape that reaches it and the derivation of that shape from the
dispatch condition in csrc/.  It is the single place that says which test covers which branch:

  * a row with `covered_by` points at an existing parametrised case that already checks the branch exactly (the pinned CONV_CASES
    of test_ops_gpu.py, the CONVT_CASES that carry an assertion, and the fused-statistics tests); `shape` is then that test's case
    tuple.  Those tests read the kernel name they assert from here (expect_kernels, covered_kernel), except test_convT3d_fwd_bwd,
    which states its two names itself;
  * every other row names a key of SHAPES, and test_conv_dispatch_gpu.py runs that shape in each of the row's dtypes: kernel name,
    bit-exact integer pass, per-element fp64 bound.

test_conv_dispatch_cpu.py holds the ledger against the code on the CPU: rx_ch_choose swept, every row put to the route of its entry
point (csrc/rx_gather_plan.h, csrc/rx_wgrad_plan.h), the kernel names read from the sources.

Entry points: conv3d_fwd, conv3d_fwd_stats, conv3d_bwd_data (accumulate 0), conv3d_bwd_data+ (accumulate 1), conv3d_bwd_data_instats
(and +), conv3d_bwd_weight, convT3d_fwd, convT3d_bwd_data (and +), convT3d_bwd_weight.
`flags` (halo rows) = (FLIP, STATS, ACC, BS) of the instantiation rx_ch_choose names; `sub` = the split count or run-time branch no
kernel name shows, with its arithmetic in `why`.  Tiles: 3x3x3 stride-1 layers are cut into 256-voxel tiles (4x4x16 when X >= 16,
4x8x8 when X = 8); `pairs` = tiles x output-channel blocks."""
import collections

HALF = ("bfloat16", "float16")
F32 = ("float32",)
ALL = HALF + F32
K3, K133, K1 = (3, 3, 3), (1, 3, 3), (1, 1, 1)
S1, S2, S122 = (1, 1, 1), (2, 2, 2), (1, 2, 2)

# the shapes test_conv_dispatch_gpu.py runs: kind, batch, Ci, Co, input extents, kernel (conv) and stride
Shape = collections.namedtuple("Shape", "kind n ci co dims k s dtypes")
SHAPES = {
    # the halo branches that had only a recorded digest (conv_halo_cases.SHAPES, batch 2 as derived there)
    "D1": Shape("conv", 2, 32, 32, (16, 32, 48), K3, S1, ALL),
    "D2": Shape("conv", 2, 128, 32, (16, 32, 48), K3, S1, HALF),     # (fp32: conv_halo32 / conv_halo_kernel<64>, rows of D1 / E4)
    "E1": Shape("conv", 2, 32, 64, (48, 32, 8), K3, S1, ALL),
    "E2": Shape("conv", 2, 32, 256, (32, 32, 8), K3, S1, ALL),
    "E3": Shape("conv", 2, 64, 64, (48, 32, 8), K3, S1, ALL),       # E1 / E2 as data gradients: the run-time `flip` of conv_halo_kernel
    "E4": Shape("conv", 2, 256, 32, (32, 32, 8), K3, S1, ALL),
    "B2": Shape("conv", 2, 64, 128, (14, 32, 64), K3, S1, ALL),
    # the gather kernels, batch 1
    "I1": Shape("conv", 1, 64, 32, (4, 4, 8), K133, S1, ALL),
    "I3": Shape("conv", 1, 64, 64, (8, 8, 16), K3, S2, ALL),
    "I4": Shape("conv", 1, 32, 64, (3, 8, 8), K133, S1, ALL),
    "I5": Shape("conv", 1, 64, 64, (3, 8, 8), K3, S1, ALL),
    "I6": Shape("conv", 1, 32, 64, (4, 8, 16), K3, S122, ALL),
    "I7": Shape("conv", 1, 32, 32, (3, 8, 8), K133, S1, ALL),
    "FAT1": Shape("conv", 1, 1024, 2048, (8, 16, 16), K1, S1, ALL),
    # the weight-gradient halo kernels' split / reduce forms
    "W1": Shape("conv", 1, 32, 32, (4, 4, 16), K3, S1, HALF),
    "W2": Shape("conv", 1, 32, 32, (4, 8, 32), K3, S1, ALL),
    "W3": Shape("conv", 1, 32, 32, (16, 16, 8), K3, S1, ALL),
    "T1": Shape("convT", 1, 64, 64, (2, 4, 4), None, S2, ALL),
}

Row = collections.namedtuple("Row", "entry kernel dtypes shape why sub flags covered_by", defaults=(None, None, None))
OPS = "tests/test_ops_gpu.py::"
PIN = OPS + "test_conv3d_fwd_bwd"
FWD, STATS, DX, DXA, BS, BSA, DW = ("conv3d_fwd", "conv3d_fwd_stats", "conv3d_bwd_data", "conv3d_bwd_data+", "conv3d_bwd_data_instats",
                                    "conv3d_bwd_data_instats+", "conv3d_bwd_weight")
TFWD, TDX, TDXA, TDW = "convT3d_fwd", "convT3d_bwd_data", "convT3d_bwd_data+", "convT3d_bwd_weight"

# the CONV_CASES of test_ops_gpu.py whose kernels are pinned there (n = 2)
P_A = (32, 32, (30, 36, 64), K3, S1)
P_B1 = (64, 64, (14, 32, 64), K3, S1)
P_C = (64, 96, (14, 32, 32), K3, S1)
P_F1 = (256, 256, (4, 4, 4), K3, S1)
P_F512 = (512, 512, (4, 4, 4), K3, S1)
P_F388 = (512, 512, (3, 8, 8), K3, S1)
P_S2 = (128, 64, (32, 32, 64), K3, S2)
P_S2R = (128, 64, (24, 40, 72), K3, S2)
P_PW = (64, 128, (12, 20, 18), K1, S1)

ROWS = [
    # ---- conv_halo32p_kernel (16 bit): Ci = Co = 32, tiles >= 512.  2 * 8 * 9 * 4 = 576 tiles
    Row(FWD, "conv_halo32p_kernel", HALF, P_A, "NT = 2*8*9*4 = 576 >= 512, 32 -> 32", flags=(0, 0, 0, 0), covered_by=PIN),
    Row(DX, "conv_halo32p_kernel", HALF, P_A, "the same query with flip", flags=(1, 0, 0, 0), covered_by=PIN),
    Row(DXA, "conv_halo32p_kernel", HALF, P_A, "flip and accumulate: ACC", flags=(1, 0, 1, 0), covered_by=PIN),
    Row(STATS, "conv_halo32p_kernel", HALF, (32, 32, (30, 36, 64)), "n = 3: 864 tiles; room for [3][1024][2][32] floats: STATS",
        flags=(0, 1, 0, 0), covered_by=OPS + "test_conv3d_fwd_stats"),
    Row(BS, "conv_halo32p_kernel", HALF, (32, (30, 36, 64)), "n = 3, flip with the backward sums: BS", flags=(1, 0, 0, 1),
        covered_by=OPS + "test_conv3d_bwd_data_instats"),
    Row(BSA, "conv_halo32p_kernel", HALF, (32, (30, 36, 64)), "the same with accumulate: ACC and BS", flags=(1, 0, 1, 1),
        covered_by=OPS + "test_conv3d_bwd_data_instats"),
    # ---- conv_halo64ws_kernel (16 bit): Co % 64 == 0, tiles * Co/64 >= 256
    Row(FWD, "conv_halo64ws_kernel", HALF, P_B1, "NT = 2*4*8*4 = 256, Co/64 = 1: 256 pairs", sub="grid_y=1", flags=(0, 0, 0, 0), covered_by=PIN),
    Row(DX, "conv_halo64ws_kernel", HALF, P_B1, "the same query with flip", sub="grid_y=1", flags=(1, 0, 0, 0), covered_by=PIN),
    Row(DXA, "conv_halo64ws_kernel", HALF, P_B1, "flip and accumulate below 2 GiB: ACC (old values prefetched)", sub="grid_y=1", flags=(1, 0, 1, 0),
        covered_by=PIN),
    Row(STATS, "conv_halo64ws_kernel", HALF, (64, 64, (14, 32, 64)), "room and DMA: STATS", sub="grid_y=1", flags=(0, 1, 0, 0),
        covered_by=OPS + "test_conv3d_fwd_stats"),
    Row(BS, "conv_halo64ws_kernel", HALF, (64, (14, 30, 64)), "n = 3, whole-row stores: BS on the producer waves", sub="grid_y=1",
        flags=(1, 0, 0, 1),
        covered_by=OPS + "test_conv3d_bwd_data_instats"),
    Row(BSA, "conv_halo64ws_kernel", HALF, (64, (14, 30, 64)), "the same with accumulate", sub="grid_y=1", flags=(1, 0, 1, 1),
        covered_by=OPS + "test_conv3d_bwd_data_instats"),
    # B2: two 64-channel blocks share each tile (grid_y = 2): per = 4 tiles a workgroup instead of 2
    Row(FWD, "conv_halo64ws_kernel", HALF, "B2", "NT = 256, Co/64 = 2: 512 pairs, cap 256/2 = 128 workgroups: grid 64 x 2, per 4",
        sub="grid_y=2", flags=(0, 0, 0, 0)),
    Row(STATS, "conv_halo64ws_kernel", HALF, "B2", "the same launch with STATS: chunks = wgs_s * 4 = 128 a sample", sub="grid_y=2",
        flags=(0, 1, 0, 0)),
    # ---- conv_halo32ws_kernel (16 bit): 32-channel blocks, Ci >= 64, pairs >= 256
    Row(FWD, "conv_halo32ws_kernel", HALF, P_C, "NT = 2*4*8*2 = 128, Co/32 = 3: 384 pairs, Ci = 64", flags=(0, 0, 0, 0), covered_by=PIN),
    Row(DX, "conv_halo32ws_kernel", HALF, P_C, "flip: Ci = 96, Co/32 = 2: 256 pairs", flags=(1, 0, 0, 0), covered_by=PIN),
    Row(DXA, "conv_halo32ws_kernel", HALF, P_C, "flip and accumulate: ACC", flags=(1, 0, 1, 0), covered_by=PIN),
    Row(STATS, "conv_halo32ws_kernel", HALF, (256, 256, (16, 16, 16)), "NT = 2*4*4*1 = 32, Co/32 = 8: 256 pairs: STATS",
        flags=(0, 1, 0, 0), covered_by=OPS + "test_conv3d_fwd_stats"),
    # ---- conv_halo32_kernel: 4x4x16 tiles, 32-channel blocks, what the persistent kernels leave
    Row(FWD, "conv_halo32_kernel", ALL, "D1", "NT = 2*4*8*3 = 192 >= 192 pairs, < 512 tiles and Ci = 32 < 64", flags=(0, 0, 0, 0)),
    Row(DX, "conv_halo32_kernel", ALL, "D1", "the same query with flip: FLIP", flags=(1, 0, 0, 0)),
    Row(DXA, "conv_halo32_kernel", ALL, "D1", "accumulate is a run-time flag of the FLIP instantiation", sub="g.accumulate=1",
        flags=(1, 0, 0, 0)),
    Row(STATS, "conv_halo32_kernel", HALF, "D2", "NT = 192 pairs < 256 keeps it off conv_halo32ws, Ci = 128 = 4 chunks of 32, "
        "96 tiles a sample * 4 <= 1024: STATS", flags=(0, 1, 0, 0)),
    Row(BS, "conv_halo32_kernel", ALL, "D1", "conv_halo32 has no BS instantiation: not fused, m12 untouched", sub="not fused",
        flags=(1, 0, 0, 0)),
    # D2 backwards is a 32 -> 128 launch: one input-channel chunk on conv_halo64ws, two output blocks, backward sums
    Row(DX, "conv_halo64ws_kernel", HALF, "D2", "flip: Ci = 32, Co = 128: NT * 2 = 384 >= 256", sub="grid_y=2", flags=(1, 0, 0, 0)),
    Row(DXA, "conv_halo64ws_kernel", HALF, "D2", "the same with accumulate", sub="grid_y=2", flags=(1, 0, 1, 0)),
    Row(BS, "conv_halo64ws_kernel", HALF, "D2", "the same with the backward sums", sub="grid_y=2", flags=(1, 0, 0, 1)),
    Row(BSA, "conv_halo64ws_kernel", HALF, "D2", "the same with both", sub="grid_y=2", flags=(1, 0, 1, 1)),
    # ---- conv_halo_kernel<BN>: the generic tile (4x8x8 here); flip and accumulate are run-time
    Row(FWD, "conv_halo_kernel<32>", ALL, "E1", "X = 8: tile 4x8x8; NT = 2*12*4*1 = 96, Co = 64 but 96 < 256 -> BN 32: 192 pairs",
        flags=(0, 0, 0, 0)),
    Row(FWD, "conv_halo_kernel<64>", ALL, "E2", "tile 4x8x8; NT = 2*8*4*1 = 64, Co/64 = 4: 256 pairs", flags=(0, 0, 0, 0)),
    Row(DX, "conv_halo_kernel<32>", ALL, "E3", "64 -> 64 at E1's extents: 192 pairs of 32 channels both ways", sub="g.flip=1",
        flags=(0, 0, 0, 0)),
    Row(DXA, "conv_halo_kernel<32>", ALL, "E3", "the same with accumulate", sub="g.flip=1 g.accumulate=1", flags=(0, 0, 0, 0)),
    Row(DX, "conv_halo_kernel<64>", ALL, "E4", "E2 backwards: dy 32 -> dx 256 channels, 64 * 4 = 256 pairs", sub="g.flip=1",
        flags=(0, 0, 0, 0)),
    Row(DXA, "conv_halo_kernel<64>", ALL, "E4", "the same with accumulate", sub="g.flip=1 g.accumulate=1", flags=(0, 0, 0, 0)),
    Row(FWD, "conv_halo_kernel<64>", F32, "B2", "fp32 has no wave-specialised kernel: 4x4x16 tiles on the generic one, 512 pairs",
        sub="tile 4x4x16", flags=(0, 0, 0, 0)),
    # ---- igemm_kernel<BM,BN>: BM = 128 iff voxels per phase <= 128, BN = 64 iff Co % 64 == 0.  ks: rx_gather_choose (csrc/rx_gather_plan.h)
    Row(FWD, "igemm_kernel<128,32>", ALL, "I1", "128 voxels, Co = 32; 1 workgroup, nkt = 9*64/32 = 18 >= 16: ks = min(512, 18/4) = 4 "
        "(fp32: nkt 36, ks 9)", sub={"ks": {"half": 4, "float32": 9}}),
    Row(DX, "igemm_kernel<128,64>", ALL, "I1", "dx has 64 channels; 16 bit: nkt = 9*32/32 = 9 < 16: ks = 1 (fp32: nkt 18, ks 4)",
        sub={"ks": {"half": 1, "float32": 4}}),
    Row(DXA, "igemm_kernel<128,64>", ALL, "I1", "the same with accumulate", sub={"ks": {"half": 1, "float32": 4}}),
    Row(FWD, "igemm_kernel<128,64>", ALL, "I3", "stride 2: 4*4*8 = 128 output voxels; nkt = 27*2 = 54: ks = min(512, 13) = 13 "
        "(fp32: 27)", sub={"ks": {"half": 13, "float32": 27}, "stride": 2}),
    Row(DX, "igemm_kernel<128,64>", ALL, "I3", "stride 2: 8 parity classes of 128 voxels, 8 workgroups, nkt = 8 taps * 2 = 16: "
        "ks = min(64, 4) = 4 (fp32: 8)", sub={"ks": {"half": 4, "float32": 8}, "stride": 2}),
    Row(DXA, "igemm_kernel<128,64>", ALL, "I3", "the same with accumulate", sub={"ks": {"half": 4, "float32": 8}, "stride": 2}),
    Row(FWD, "igemm_kernel<128,64>", ALL, "I6", "stride (1,2,2): 4*4*8 = 128 output voxels, Co = 64; nkt = 27: ks = 6 (fp32: 13)",
        sub={"ks": {"half": 6, "float32": 13}, "stride": (1, 2, 2)}),
    Row(DX, "igemm_kernel<128,32>", ALL, "I6", "stride (1,2,2): 4 classes of 128 voxels, dx has 32 channels; nkt = 12 taps * 2 = 24: "
        "ks = min(128, 6) = 6 (fp32: 12)", sub={"ks": {"half": 6, "float32": 12}, "stride": (1, 2, 2)}),
    Row(DXA, "igemm_kernel<128,32>", ALL, "I6", "the same with accumulate", sub={"ks": {"half": 6, "float32": 12}, "stride": (1, 2, 2)}),
    Row(FWD, "igemm_kernel<256,64>", ALL, "I4", "192 voxels > 128, Co = 64; 16 bit: nkt = 9 < 16: ks = 1 (fp32: 18, ks 4)",
        sub={"ks": {"half": 1, "float32": 4}}),
    Row(DX, "igemm_kernel<256,32>", ALL, "I4", "dx has 32 channels; nkt = 9*2 = 18: ks = 4 (fp32: 9)",
        sub={"ks": {"half": 4, "float32": 9}}),
    Row(DXA, "igemm_kernel<256,32>", ALL, "I4", "the same with accumulate", sub={"ks": {"half": 4, "float32": 9}}),
    Row(FWD, "igemm_kernel<256,32>", ALL, "I7", "192 voxels, Co = 32; 16 bit: nkt = 9: ks = 1 (fp32: 4)",
        sub={"ks": {"half": 1, "float32": 4}}),
    Row(FWD, "igemm_kernel<256,64>", ALL, "I5", "1 tile of 4x8x8 = 2 pairs < 192 leaves the halo kernels; 192 voxels; 64 channels are "
        "no multiple of the fat kernel's 128; nkt = 54: ks = 13 -- in fp32 (nkt 108, ks 27) split-K is the only route for deep layers",
        sub={"ks": {"half": 13, "float32": 27}}),
    Row(DX, "igemm_kernel<256,64>", ALL, "I5", "the same backwards", sub={"ks": {"half": 13, "float32": 27}}),
    Row(DXA, "igemm_kernel<256,64>", ALL, "I5", "the same with accumulate", sub={"ks": {"half": 13, "float32": 27}}),
    Row(FWD, "igemm_kernel<256,64>", F32, "FAT1", "fp32 at FAT1: 8 row tiles * 32 blocks = 256 workgroups >= 192: ks = 1",
        sub={"ks": {"float32": 1}}),
    # ---- igemm_fat_kernel (16 bit): Ci % 128 == 0, Co % 64 == 0, n * voxels <= 2048, >= 8 K steps
    Row(FWD, "igemm_fat_kernel", HALF, P_F1, "NV = 128: 1 row tile * 4 blocks; 54 steps: ks = min(128, 13) = 13", sub={"ks": {"half": 13}},
        covered_by=PIN),
    Row(DX, "igemm_fat_kernel", HALF, P_F1, "the same backwards", sub={"ks": {"half": 13}}, covered_by=PIN),
    Row(FWD, "igemm_fat_kernel", HALF, P_F512, "NV = 128, 8 blocks; 108 steps: ks = min(64, 27) = 27", sub={"ks": {"half": 27}},
        covered_by=PIN),
    Row(DX, "igemm_fat_kernel", HALF, P_F512, "the same backwards", sub={"ks": {"half": 27}}, covered_by=PIN),
    Row(FWD, "igemm_fat_kernel", HALF, P_F388, "NV = 384: 3 row tiles * 8 blocks: ks = min(22, 27) = 22", sub={"ks": {"half": 22}},
        covered_by=PIN),
    Row(DX, "igemm_fat_kernel", HALF, P_F388, "the same backwards", sub={"ks": {"half": 22}}, covered_by=PIN),
    Row(FWD, "igemm_fat_kernel", HALF, "FAT1", "ks <= steps / 4 and steps >= 8, so ks = 1 needs 512 workgroups without a split: "
        "2048 voxels = 16 row tiles, Co = 2048 = 32 blocks; 1x1x1, Ci = 1024: 8 steps", sub={"ks": {"half": 1}}),
    Row(DX, "igemm_fat_kernel", HALF, "FAT1", "backwards: 16 * 16 blocks = 256 workgroups, 16 steps: ks = min(2, 4) = 2",
        sub={"ks": {"half": 2}}),
    Row(DXA, "igemm_fat_kernel", HALF, "FAT1", "the same with accumulate", sub={"ks": {"half": 2}}),
    # ---- dgrad_s2p_kernel, pointwise_kernel (16 bit)
    Row(DX, "dgrad_s2p_kernel", HALF, P_S2, "64 dY channels, even extents, NT * Ci/32 = 256 * 4", covered_by=PIN),
    Row(DX, "dgrad_s2p_kernel", HALF, P_S2R, "the same with ragged dY tiles", sub="ragged", covered_by=PIN),
    Row(FWD, "pointwise_kernel", HALF, P_PW, "1x1x1, 2 * 4320 voxels >= 4096", covered_by=PIN),
    Row(DX, "pointwise_kernel", HALF, P_PW, "the same backwards", covered_by=PIN),
    Row(TFWD, "pointwise_kernel", HALF, (64, 32, (12, 18, 20), S2), "8 taps * 32 * (128 + 16) B = 36 KB of weights, 8640 voxels",
        covered_by=OPS + "test_convT3d_fwd_bwd"),
    # ---- wgrad_kernel<BR,BC>: BR = 64 iff Co % 64 == 0, BC = 64 iff Ci % 64 == 0; S: rx_wgrad_split (csrc/rx_wgrad_plan.h)
    Row(DW, "wgrad_kernel<32,64>", ALL, "I1", "1x3x3 is not for the halo kernels; Co = 32, Ci = 64; 2 K tiles: S = 1", sub={"S": 1}),
    Row(DW, "wgrad_kernel<64,32>", ALL, "I4", "Co = 64, Ci = 32; 3 K tiles: S = 1", sub={"S": 1}),
    Row(DW, "wgrad_kernel<32,32>", ALL, "I7", "Co = Ci = 32; 3 K tiles: S = 1", sub={"S": 1}),
    Row(DW, "wgrad_kernel<64,64>", F32, "I5", "fp32 never takes the halo kernels; 3 K tiles: S = 1", sub={"S": 1}),
    Row(DW, "wgrad_kernel<32,32>", F32, "W2", "fp32: 16 K tiles / 4: S = 4 -> wgrad_reduce", sub={"S": 4, "reduce": "wgrad_reduce"}),
    Row(DW, "wgrad_kernel<32,32>", F32, "W3", "fp32: 32 K tiles / 4: S = 8 -> wgrad_reduce_manysplits",
        sub={"S": 8, "reduce": "wgrad_reduce_manysplits"}),
    Row(TDW, "wgrad_kernel<64,64>", ALL, "T1", "32 coarse voxels < 32768; 64 -> 64; 1 K tile: S = 1", sub={"S": 1}),
    # ---- wgrad_halo_kernel / wgrad_halo16ws_kernel (16 bit): S == 1 writes dw, S > 1 writes slabs and reduces them
    Row(DW, "wgrad_halo_kernel", HALF, "I5", "tile 4x8x8, NT = 1: S = min(512/4, 1) = 1: dw written directly", sub={"S": 1}),
    Row(DW, "wgrad_halo_kernel", HALF, P_F512, "256 panel pairs fill the chip: S = 1", sub={"S": 1}, covered_by=PIN),
    Row(DW, "wgrad_halo_kernel", HALF, P_F388, "256 panel pairs: S = 1, two ragged 4x8x8 tiles a workgroup", sub={"S": 1}, covered_by=PIN),
    Row(DW, "wgrad_halo_kernel", HALF, P_F1, "tile 4x4x4, NT = 2, 64 pairs: S = min(8, 2) = 2 -> wgrad_reduce",
        sub={"S": 2, "reduce": "wgrad_reduce"}, covered_by=PIN),
    Row(DW, "wgrad_halo16ws_kernel", HALF, P_B1, "NT = 256, 4 pairs: S = 128", sub={"S": 128, "reduce": "wgrad_reduce_manysplits"},
        covered_by=PIN),
    Row(DW, "wgrad_halo_kernel", HALF, "I3", "stride 2: 64-voxel tile 2x4x8, halo 5*9*17 = 765 <= 768; NT = 2: S = 2 -> wgrad_reduce",
        sub={"S": 2, "reduce": "wgrad_reduce", "stride": 2}),
    Row(DW, "wgrad_halo_kernel", HALF, "I6", "stride (1,2,2): tile 2x4x8, halo 4*9*17; NT = 2: S = 2 -> wgrad_reduce",
        sub={"S": 2, "reduce": "wgrad_reduce", "stride": (1, 2, 2)}),
    Row(DW, "wgrad_halo_kernel", HALF, "W3", "tile 4x8x8, NT = 4*2*1 = 8, 1 panel pair: S = min(512, 8) = 8 -> wgrad_reduce_manysplits",
        sub={"S": 8, "reduce": "wgrad_reduce_manysplits"}),
    Row(DW, "wgrad_halo16ws_kernel", HALF, "W1", "one 4x4x16 tile: S = min(512, NT = 1) = 1: dw written directly", sub={"S": 1}),
    Row(DW, "wgrad_halo16ws_kernel", HALF, "W2", "NT = 1*2*2 = 4: S = 4 -> wgrad_reduce", sub={"S": 4, "reduce": "wgrad_reduce"}),
    Row(DW, "wgrad_halo16ws_kernel", HALF, "D1", "NT = 192, 1 pair: 192 < 4096 -> target 512: S = 192 -> wgrad_reduce_manysplits",
        sub={"S": 192, "reduce": "wgrad_reduce_manysplits"}),
    Row(DW, "wgrad_halo16ws_kernel", HALF, P_A, "NT = 576: S = 288", sub={"S": 288, "reduce": "wgrad_reduce_manysplits"}, covered_by=PIN),
    # ---- transposed conv
    Row(TFWD, "igemm_kernel<128,64>", ALL, "T1", "32 voxels < 4096 leaves pointwise_kernel: 8 one-tap phases of 32 voxels; nkt = 2: ks = 1",
        sub={"ks": {"half": 1, "float32": 1}}),
    Row(TDX, "igemm_kernel<128,64>", ALL, "T1", "one phase of 8 taps; nkt = 8*2 = 16: ks = 4 (fp32: 8)",
        sub={"ks": {"half": 4, "float32": 8}}),
    Row(TDXA, "igemm_kernel<128,64>", ALL, "T1", "the same with accumulate", sub={"ks": {"half": 4, "float32": 8}}),
    Row(TDW, "convT_wgrad_kernel", HALF, (64, 32, (16, 32, 40), S2), "2 * 20480 coarse voxels >= 32768, 2 x 1 panels",
        covered_by=OPS + "test_convT3d_fwd_bwd"),
]

# Instantiations no test of a few seconds can reach: each needs an operand past the 32-bit buffer range (or an alignment torch never
# hands out).  test_conv_halo_plan_cpu.py and test_conv_dispatch_cpu.py execute the planners' side of these on the CPU.
UNREACHABLE = {
    "conv_halo64ws_kernel<XDMA=false>": "input of n * voxels * ld * 2 bytes >= 0x7fffff00 (2 GiB): the register-staged producers",
    "wgrad_halo16ws_kernel<DMA=false>": "dy or x of >= 2 GiB: the register-staged producers",
    "conv_halo32_kernel in place of conv_halo32ws_kernel": "a >= 64-channel input of >= 2 GiB",
}


def rows_for(shape_key, dtype_name):
    return [r for r in ROWS if r.shape == shape_key and dtype_name in r.dtypes]


def expect_kernels(rows=None):
    """{CONV_CASES tuple: (fwd, bwd-data, bwd-weight) kernel or None} for test_conv3d_fwd_bwd's 16-bit pins: the rows that point at it"""
    out = {}
    for r in (ROWS if rows is None else rows):
        if r.covered_by == PIN and r.entry in (FWD, DX, DW):
            cur = out.setdefault(r.shape, [None, None, None])
            i = (FWD, DX, DW).index(r.entry)
            assert cur[i] in (None, r.kernel), (r.shape, r.entry)
            cur[i] = r.kernel
    return {k: tuple(v) for k, v in out.items()}


def covered_kernel(test, shape, entry):
    """the kernel (16-bit modes) of the row that points at case `shape` of tests/test_ops_gpu.py::`test` for `entry`; None: no such row"""
    hit = [r.kernel for r in ROWS if r.covered_by == OPS + test and r.shape == shape and r.entry == entry]
    assert len(hit) <= 1, (test, shape, entry)
    return hit[0] if hit else None
