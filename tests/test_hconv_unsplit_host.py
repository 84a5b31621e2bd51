"""Host logic of the unsplit 4x16-pixel x 128-channel tile of hconv2_kernel (csrc/hconv.hip cgd_hconv_tile_m, csrc/gemm.hip), without a GPU through
cgd_op_plan_conv: where the launcher picks it by itself, and that everything else stays on the path it had."""
import ctypes as C

from cgd_amd import lib

HCONV, WCONV, KCONV = 512, 515, 516


def plan(H, ci, co, Bn=1, W=None, precision=1, num_cu=256, var=0, stats=0, gnb=0):
    out = (C.c_int * 5)()
    rc = lib.load().cgd_op_plan_conv(Bn, H, H if W is None else W, ci, co, precision, num_cu, var, stats, gnb, out)
    return rc, tuple(out)  # (kernel, tile code, split-K, workgroups, pixels per hconv2 tile)


def test_the_launcher_picks_the_unsplit_tile_only_where_it_leaves_records_and_fills_the_chip():
    # the three 64x64 shapes of BASELINE config 2, forward (stats) and dgrad (gnb): one slice, one 64-pixel tile per CU
    for ci in (512, 768, 1024):
        assert plan(64, ci, 512, stats=1) == (0, (1, HCONV, 1, 256, 64))
        assert plan(64, ci, 512, gnb=1) == (0, (1, HCONV, 1, 256, 64))
    assert plan(64, 512, 1024, stats=1) == (0, (1, HCONV, 1, 256, 128))  # 256 tiles of 128 pixels already: nothing to split
    # nobody wants records: the two slices of before (what cgd_op_plan reports, too)
    assert plan(64, 512, 512) == (0, (1, HCONV, 2, 256, 128))
    out4 = (C.c_int * 4)()
    assert lib.load().cgd_op_plan(1, 4096, 512, 0, 64, 64, 512, 0, 1, 256, out4) == 0 and tuple(out4) == (1, HCONV, 2, 256)
    # plain-bf16 and exact-fp32 contexts keep their paths
    assert plan(64, 512, 512, precision=2, stats=1) == (0, (1, HCONV, 2, 256, 128))
    assert plan(64, 512, 512, precision=0, stats=1)[1][0] == 0
    # a Cout that is no multiple of 128 stays on the 128-pixel tile, also when the variant is forced
    assert plan(64, 512, 320, stats=1)[1][4] == 128 and plan(64, 512, 320, var=8, stats=1)[1][4] == 128
    assert plan(64, 512, 192, var=8)[1][4] == 128
    # fewer CUs: the 128-pixel tiling fills the chip; more samples: as well
    assert plan(64, 512, 512, num_cu=64, stats=1) == (0, (1, HCONV, 1, 128, 128))
    assert plan(64, 512, 512, Bn=2, stats=1) == (0, (1, HCONV, 1, 256, 128))
    # too few 64-pixel tiles for the chip: the split stays (a 64x32 map: 128 tiles of 64 pixels x 4 channel tiles... = 256 would fill it; 48x32 does not)
    assert plan(48, 512, 512, W=32, stats=1)[1][4] == 128
    # the other levels are untouched: Winograd kernel from 128^2, weight-streaming kernel up to 32^2
    assert plan(128, 256, 256, stats=1)[1][1] == WCONV and plan(32, 512, 512, stats=1)[1][1] == KCONV
    # other tile variants forced: no automatic choice
    assert plan(64, 512, 512, var=1, stats=1)[1][4] == 256
    # forced (tests, benchmarks): any shape with Cout a multiple of 128, never split by the launcher
    assert plan(64, 512, 512, var=8) == (0, (1, HCONV, 1, 256, 64)) and plan(64, 512, 256, var=8) == (0, (1, HCONV, 1, 128, 64))
    assert lib.load().cgd_op_plan_conv(1, 64, 64, 512, 512, 1, 256, 0, 1, 0, None) == -3
