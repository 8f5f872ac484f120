"""Pass 1's document pools (fluidframework_amd/csrc/pool_layout.h, the rule
mte_load_docs lays a batch out by), without a GPU: the header is host code
alone, so a small program around it is compiled with the host compiler and
prints the layout of every case.

  * every flat document is in exactly one pool, in order;
  * pool sizes differ by at most one and never exceed 32 (kPoolMax);
  * a batch that fits the chip at one document per wave gets one per wave
    (pools of at most 4 = kPairsPerBlock documents);
  * a larger batch gets one pool per resident workgroup until the pools are
    full, then more pools.
"""
import os
import shutil
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "fluidframework_amd", "csrc")
WPB, CAP = 4, 32

MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include "pool_layout.h"
int main(int argc, char** argv) {
  // nf cus waves wpb cap -> "n_pools pool_max" and the first[] table
  for (int i = 1; i + 4 < argc; i += 5) {
    const mte::PoolLayout L = mte::pool_layout((uint32_t)std::strtoul(argv[i], 0, 10), (uint32_t)std::atoi(argv[i + 1]),
                                               (uint32_t)std::atoi(argv[i + 2]), (uint32_t)std::atoi(argv[i + 3]),
                                               (uint32_t)std::atoi(argv[i + 4]));
    std::printf("%u %u", L.n_pools, L.pool_max);
    for (uint32_t f : L.first) std::printf(" %u", f);
    std::printf("\n");
  }
  return 0;
}
"""


def cases():
    out = []
    for cus in (1, 256, 304):
        for w in (5, 6):
            resident = cus * 4 * w
            pools = resident // WPB
            for nf in (0, 1, resident - 1, resident, resident + 1, 2 * resident - 1, CAP * pools, CAP * pools + 1,
                       100000):
                out.append((nf, cus, w))
    return out


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("pools")
    src, exe = d / "pools_main.cpp", d / "pools_main"
    src.write_text(MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", str(exe), str(src)],
                   check=True)
    args = [str(x) for nf, cus, w in cases() for x in (nf, cus, w, WPB, CAP)]
    lines = subprocess.run([str(exe)] + args, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(cases())
    res = {}
    for case, line in zip(cases(), lines):
        v = [int(x) for x in line.split()]
        res[case] = (v[0], v[1], v[2:])
    return res


@pytest.mark.parametrize("nf,cus,w", cases())
def test_pool_layout(layouts, nf, cus, w):
    n_pools, pool_max, first = layouts[(nf, cus, w)]
    resident = cus * 4 * w
    assert len(first) == n_pools + 1
    # consecutive runs that cover [0, nf): every document in exactly one pool
    assert first[0] == 0 and first[-1] == nf
    sizes = [b - a for a, b in zip(first, first[1:])]
    assert all(s >= 0 for s in sizes)
    if nf == 0:
        assert n_pools == 0 and pool_max == 0
        return
    assert min(sizes) >= 1  # no empty workgroup
    assert max(sizes) - min(sizes) <= 1
    assert max(sizes) == pool_max <= CAP
    if nf <= resident:
        # one document per wave, on as few workgroups as hold them
        assert pool_max <= WPB
        assert n_pools == -(-nf // WPB)
    else:
        # every resident workgroup has a pool; more only when they are full
        assert pool_max > WPB
        assert n_pools == max(resident // WPB, -(-nf // CAP))
