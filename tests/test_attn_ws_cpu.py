"""CPU check of the attention-backward workspace gate (attn_ws.h).

A stand-alone C++ program (host compiler only) includes the header and
prints, for every (b, h, s, limit) given, the workspace byte count and the
gate's decision. The sizes go past 2^31 and 2^32, so a 32-bit product
anywhere in the header would show up here."""

import os
import shutil
import subprocess

import pytest

HIP_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                       "fms_fsdp_amd", "ops", "hip")

GIB = 1 << 30
DEFAULT = 4 * GIB

# (b, h, s, limit_bytes)
CASES = [
    (2, 32, 4096, 4 * GIB),
    (2, 32, 4096, 2 * GIB),
    (2, 32, 4096, 2 * GIB - 1),
    (1, 32, 32768, DEFAULT),
    (1, 64, 65536, DEFAULT),
    (2, 32, 4096, 0),
    (1, 1, 128, 0),
    (1, 2, 128, DEFAULT),
]

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "attn_ws.h"
int main(int argc, char** argv) {
  printf("default_mb %lld\n", (long long)ATTN_BWD_WS_DEFAULT_MB);
  for (int i = 1; i + 3 < argc; i += 4) {
    const long long b = atoll(argv[i]), h = atoll(argv[i + 1]),
                    s = atoll(argv[i + 2]), lim = atoll(argv[i + 3]);
    printf("%lld %lld %lld %lld %lld %d\n", b, h, s, lim,
           (long long)attn_bwd_ws_bytes(b, h, s),
           attn_bwd_use_workspace(b, h, s, lim) ? 1 : 0);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def gate(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++")
                if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    d = tmp_path_factory.mktemp("attn_ws")
    src, exe = d / "main.cpp", d / "attn_ws_main"
    src.write_text(MAIN)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror",
                           "-I", HIP_DIR, str(src), "-o", str(exe)])
    args = [str(v) for case in CASES for v in case]
    out = subprocess.check_output([str(exe)] + args, text=True).splitlines()
    table = {"default_mb": int(out[0].split()[1])}
    for line in out[1:]:
        b, h, s, lim, nbytes, use = map(int, line.split())
        table[(b, h, s, lim)] = (nbytes, bool(use))
    assert len(table) == len(CASES) + 1
    return table


def test_default_is_4_gib(gate):
    assert gate["default_mb"] * (1 << 20) == DEFAULT


@pytest.mark.parametrize("case", CASES, ids=str)
def test_byte_count_is_exact(gate, case):
    b, h, s, _ = case
    assert gate[case][0] == b * h * s * s * 2


def test_benchmark_shape_uses_workspace_boundary_inclusive(gate):
    assert gate[(2, 32, 4096, 4 * GIB)][1]
    assert gate[(2, 32, 4096, 2 * GIB)][0] == 2 * GIB
    assert gate[(2, 32, 4096, 2 * GIB)][1]
    assert not gate[(2, 32, 4096, 2 * GIB - 1)][1]


def test_long_sequences_are_workspace_free(gate):
    """64 GiB and 512 GiB: a 32-bit product would wrap to 0 and pass."""
    assert gate[(1, 32, 32768, DEFAULT)] == (64 * GIB, False)
    assert gate[(1, 64, 65536, DEFAULT)] == (512 * GIB, False)


def test_limit_zero_never_uses_workspace(gate):
    assert not gate[(2, 32, 4096, 0)][1]
    assert not gate[(1, 1, 128, 0)][1]
    assert gate[(1, 2, 128, DEFAULT)][1]
