"""Structure of the LDS-DMA engine's linear / PLAIN instantiations (csrc/igemm_dma.hip), from a cross-compile with build.py's
flags: no GPU needed.  Checks structure, not speed:

  * a linear / PLAIN instantiation has no integer-division sequence (v_rcp_iflag_f32: the convolution form decodes
    m -> (sample, y, x) per tile row and bid -> (m tile, n tile) with it) and uses no scratch;
  * its static instruction count is at most a quarter of the GENERIC instantiation of the same tile in the same object -- the
    kernel every launch ran before the variants existed.  (The epilogue folded to this case alone compiled to 1/15 of the generic
    one; a quarter catches a variant that still drags the generic body along.)
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (BM, BN, WGM, WGN, NS) of the three short-K tiles as launch_igemm_dma instantiates them; TERMS = 3 (bf16x3)
TILES = [(64, 64, 2, 2, 2), (128, 64, 2, 2, 3), (128, 128, 2, 2, 2)]


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled name -> (instruction count, v_rcp_iflag count, scratch bytes) of every igemm_dma_kernel in the object."""
    from audiogpt_amd import build as B
    out = str(tmp_path_factory.mktemp("isa") / "igemm_dma.s")
    cmd = [B._hipcc()] + B.FLAGS + ["--cuda-device-only", "-S", os.path.join(B.CSRC, "igemm_dma.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    table, name = {}, None
    for line in open(out):
        m = re.match(r"^(_Z\w*igemm_dma_kernel\w*):", line)
        if m:
            name = m.group(1)
            table[name] = [0, 0, None]
            continue
        if name is None:
            continue
        s = line.strip()
        if re.match(r"^[a-z][a-z_0-9]*(\s|$)", s) and line[0] in " \t":
            table[name][0] += 1
            if s.startswith("v_rcp_iflag"):
                table[name][1] += 1
        m = re.match(r"^;\s*ScratchSize:\s*(\d+)", s)
        if m:
            table[name][2] = int(m.group(1))
            name = None
    return table


def find(kernels, tile, linear, epi):
    """The instantiation <BM, BN, WGM, WGN, NS, 3, LINEAR, Epi(epi)> by its mangled template arguments."""
    args = "".join("Li%dE" % v for v in tile + (3,)) + "Lb%dE" % int(linear)
    hits = [k for k in kernels if args in k and re.search(r"EpiE%dE" % epi, k)]
    assert len(hits) == 1, (tile, linear, epi, sorted(kernels))
    return kernels[hits[0]]


@pytest.mark.parametrize("tile", TILES)
def test_linear_plain_instantiation_is_small_and_division_free(kernels, tile):
    n_plain, rcp, scratch = find(kernels, tile, True, 1)
    n_generic, rcp_generic, _ = find(kernels, tile, False, 0)
    print("tile %s: linear/PLAIN %d instructions, GENERIC %d (%d division sequences)" % (tile, n_plain, n_generic, rcp_generic))
    assert rcp == 0
    assert scratch == 0
    assert rcp_generic > 0            # (the count does see the sequence where it exists)
    assert n_plain > 100 and 4 * n_plain <= n_generic
