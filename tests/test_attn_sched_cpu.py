"""CPU check of the causal-attention workgroup mapping (attn_sched.h).

A stand-alone C++ program (host compiler only) includes the header and
prints attn_sched_map() for every linear workgroup id; the properties are
asserted here."""

import os
import shutil
import subprocess

import pytest

HIP_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                       "fms_fsdp_amd", "ops", "hip")

SHAPES = [(1, 1), (1, 2), (3, 3), (5, 12), (8, 8), (9, 16), (4, 24), (32, 64)]
BALANCED, LEGACY = 0, 1

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "attn_sched.h"
int main(int argc, char** argv) {
  if (ATTN_SCHED_BALANCED != 0 || ATTN_SCHED_LEGACY != 1) return 2;
  for (int i = 1; i + 1 < argc; i += 2) {
    const int ntile = atoi(argv[i]), nbh = atoi(argv[i + 1]);
    for (int mode = 0; mode < 2; ++mode)
      for (int heavy_low = 0; heavy_low < 2; ++heavy_low)
        for (int L = 0; L < ntile * nbh; ++L) {
          const AttnWork w = attn_sched_map(L, ntile, nbh, mode, heavy_low);
          printf("%d %d %d %d %d %d %d\n", ntile, nbh, mode, heavy_low, L,
                 w.tile, w.bh);
        }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def mapping(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("attn_sched")
    src, exe = d / "main.cpp", d / "attn_sched_main"
    src.write_text(MAIN)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I", HIP_DIR, str(src), "-o", str(exe)])
    args = [str(v) for shape in SHAPES for v in shape]
    out = subprocess.check_output([str(exe)] + args, text=True)
    table = {}
    for line in out.splitlines():
        ntile, nbh, mode, heavy_low, L, tile, bh = map(int, line.split())
        table.setdefault((ntile, nbh, mode, heavy_low), []).append((tile, bh))
        assert len(table[(ntile, nbh, mode, heavy_low)]) == L + 1
    return table


def cost(tile, ntile, heavy_low):
    return ntile - tile if heavy_low else tile + 1


@pytest.mark.parametrize("ntile,nbh", SHAPES)
@pytest.mark.parametrize("heavy_low", [0, 1])
@pytest.mark.parametrize("mode", [BALANCED, LEGACY])
def test_bijection(mapping, ntile, nbh, heavy_low, mode):
    pairs = mapping[(ntile, nbh, mode, heavy_low)]
    assert len(pairs) == ntile * nbh
    assert sorted(pairs) == [(t, b) for t in range(ntile) for b in range(nbh)]


@pytest.mark.parametrize("ntile,nbh", SHAPES)
@pytest.mark.parametrize("heavy_low", [0, 1])
def test_legacy_is_x_fastest_2d_grid(mapping, ntile, nbh, heavy_low):
    pairs = mapping[(ntile, nbh, LEGACY, heavy_low)]
    assert pairs == [(L % ntile, L // ntile) for L in range(ntile * nbh)]


@pytest.mark.parametrize("ntile,nbh", SHAPES)
@pytest.mark.parametrize("heavy_low", [0, 1])
def test_balanced_heaviest_first(mapping, ntile, nbh, heavy_low):
    costs = [cost(t, ntile, heavy_low)
             for t, _ in mapping[(ntile, nbh, BALANCED, heavy_low)]]
    assert costs[0] == ntile
    assert all(a >= b for a, b in zip(costs, costs[1:]))


@pytest.mark.parametrize("ntile,nbh", [s for s in SHAPES if s[1] % 8 == 0])
@pytest.mark.parametrize("heavy_low", [0, 1])
def test_balanced_xcd_groups_equal(mapping, ntile, nbh, heavy_low):
    pairs = mapping[(ntile, nbh, BALANCED, heavy_low)]
    group = [0] * 8
    for L, (t, bh) in enumerate(pairs):
        group[L % 8] += cost(t, ntile, heavy_low)
        # a (b,h) stays in one group: its K/V is served by one XCD's L2
        assert L % 8 == bh % 8
    assert len(set(group)) == 1, group
    assert group[0] * 8 == nbh * ntile * (ntile + 1) // 2
