"""The position-tile geometries of the GPU sweep (tests/test_gpu_tile_geometry.py), checked without a GPU: every row of
helpers.TILE_GEOMETRIES follows from its own (RL, n_q, slots, ISS_TILES) by a restatement of the upload's tiling rule, and
every k_main_g instantiation the library holds is forced by some test."""
import os
import re

import pytest

import helpers

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "insilicoseq_amd", "csrc")

# iss_kernels.hip.h: the letter tables, the substitution-test thresholds, the workgroup, a wavefront's ring of deferred lane-items
MAIN_LUT_WORDS, MAIN_MUT_WORDS, MAIN_THREADS, SLOW_RING = 512, 128, 1024, 128
LDS_BUDGET = 158 * 1024  # one workgroup per CU
MAX_TILES = 64


def _constant(name):
    text = open(os.path.join(CSRC, "iss_kernels.hip.h")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def tiling(RL, n_q, nonempty, env_tiles, guide_bits=6):
    """iss_model_upload's position tiling (iss_api_model.hip.h, fits() and main_lds_bytes()), restated: the fewest tiles whose
    tables fit the LDS of one workgroup per CU, or ISS_TILES tiles if those fit; tiles of a split start at whole 128-byte lines
    (4 superitems).  A quality row holds at most n_q distinct digits and two closing entries (a CDF ends at 1.0: its last digit
    is the sentinel's); fewer only where two thresholds share their leading 16 bits.  Returns (n_tiles, TS, last tile, ni)."""
    S = (RL + 7) // 8
    NB = max(sum(nonempty[0]), sum(nonempty[1]))
    stride_w = (1 << guide_bits) // 4 + n_q + 2
    GS = 4 * stride_w + 1

    def fits(n_tiles):
        TS = (S + n_tiles - 1) // n_tiles
        if n_tiles > 1:
            TS = (TS + 3) // 4 * 4
        TG, TP = 2 * TS, 8 * TS
        tile_words = (2 * NB * TG * GS + 3) // 4 * 4
        words = MAIN_LUT_WORDS + tile_words + MAIN_MUT_WORDS + 2 * TP * 4 + (MAIN_THREADS // 64) * SLOW_RING * 3
        return TS if 4 * words <= LDS_BUDGET else 0

    TS = fits(env_tiles) if env_tiles > 0 else 0
    for nt in range(1, S + 1):
        if TS:
            break
        TS = fits(nt)
    assert TS, "the tables do not fit the LDS"
    n_tiles = (S + TS - 1) // TS
    assert n_tiles <= MAX_TILES
    return n_tiles, TS, S - (n_tiles - 1) * TS, (TS + 3) // 4


def test_the_restatement_uses_the_kernels_constants():
    for name, value in (("MAIN_LUT_WORDS", MAIN_LUT_WORDS), ("MAIN_MUT_WORDS", MAIN_MUT_WORDS), ("MAIN_THREADS", MAIN_THREADS),
                        ("SLOW_RING", SLOW_RING), ("MAX_TILES", MAX_TILES)):
        assert _constant(name) == value, name


@pytest.mark.parametrize("geo", helpers.TILE_GEOMETRIES, ids=lambda g: g.id)
def test_every_row_follows_from_its_model(geo):
    assert helpers.TILE_GEOMETRY_ENV["ISS_GUIDE_BITS"] == "6"
    assert tiling(geo.RL, geo.n_q, geo.nonempty, geo.tiles) == (geo.n_tiles, geo.TS, geo.last, geo.ni)


def test_the_rows_reach_what_they_are_there_for():
    """The properties the sweep is built on, from the rows themselves: ni == 3 (k_main_g<3, 1>), ten iterations and more (the
    reload of the script rows, sc_gpt 2 and 3, it_bits 4 and 5), the edges of the last tile, the script's pitch limit."""
    g = {x.id: x for x in helpers.TILE_GEOMETRIES}
    ap_max_pitch = _constant("AP_MAX_PITCH")

    def pitch(x):
        return (x.RL + 7) // 8 * 8

    def sc_gpt(x):
        return (x.ni + 7) // 8

    assert [g[k].ni for k in "ABCD"] == [3, 3, 3, 3] and g["E"].ni == 1
    assert g["A"].TS % 4 == 1 and g["A"].RL % 8 == 1  # third iteration: lane 0 only, and one valid position in its superitem
    assert g["B"].RL % 8 == 0 and g["B"].TS % 4 == 0
    assert (g["C"].n_tiles, (g["C"].last + 3) // 4) == (2, 2) and (g["D"].last, g["D"].RL % 8) == (g["D"].TS, 1)
    assert (g["E"].n_tiles, g["E"].last, g["E"].RL % 8) == (2, 1, 1)
    assert [sc_gpt(g[k]) for k in "FGHIJK"] == [2, 2, 2, 2, 3, 3]
    assert [helpers.tag_iteration_bits(g[k].ni) for k in "ABCDEFGHIJK"] == [2, 2, 2, 2, 0, 4, 4, 4, 4, 5, 5]
    assert g["G"].ni == 9 and g["G"].TS % 4 == 1
    assert pitch(g["H"]) == ap_max_pitch and pitch(g["I"]) == ap_max_pitch + 8
    assert all(pitch(g[k]) <= ap_max_pitch for k in "ABCDEFGH") and all(pitch(g[k]) > ap_max_pitch for k in "IJK")
    assert g["K"].n_tiles == 1 and g["K"].ni == max(x.ni for x in helpers.TILE_GEOMETRIES)


def test_no_instantiation_without_a_test():
    """ISS_MAIN_G_LIST (iss_host_util.hip.h) == the instantiations test_gpu_grouped.FORCED forces + those of the geometry
    sweep's grouped route."""
    import test_gpu_grouped

    text = open(os.path.join(CSRC, "iss_host_util.hip.h")).read()
    line = re.search(r"^#define ISS_MAIN_G_LIST\(X\)(.*)$", text, flags=re.M).group(1)
    held = re.findall(r"X\((\d+), (\d+)\)", line)
    assert held and len(held) == len(set(held)) and "".join("X(%s, %s)" % p for p in held) == line.replace(" X", "X").strip()
    forced = {k for _, _, k in test_gpu_grouped.FORCED} | {k for _, k in helpers.TILE_GROUPED.values() if k.startswith("k_main_g")}
    assert forced == {"k_main_g<%s, %s>" % p for p in held}
    assert "k_main_g<3, 1>" not in {k for _, _, k in test_gpu_grouped.FORCED}  # (owned by the sweep)
    # a forced row names what it forces: NP is the row's ISS_MAIN_GROUP, NI its geometry's iterations per pass
    for gid, (np_, kernel) in helpers.TILE_GROUPED.items():
        geo = helpers.tile_geometry(gid)
        if (str(geo.ni), str(np_)) in held:
            assert kernel == "k_main_g<%d, %d>" % (geo.ni, np_)
        else:
            assert kernel == "k_main<false, true, false>"
