"""The streaming hint in the code object (CPU: hipcc's gfx950 assembly of launch_canopy.hip): in k_canopy_ilp_heap<SrcContig> the
16-byte pair load and the result stores must exist in a form that carries `nt` beside the plain one, and the heap-line loads
must stay plain; the kernels of general tables must keep the hinted pair load of either explicit source.  The hint is advice
and the compiler is free to drop it -- it did, by merging the hinted access of one arm of a branch with the plain one of the
other (device_common.h) -- so this is what notices."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def kernel_bodies(tmp_path_factory):
    asm = tmp_path_factory.mktemp("stream_hint") / "unit.s"
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-DST_CANOPY_PART=0",
                          "-I", os.path.join(ROOT, "include"), "--cuda-device-only", "-S", "-o", str(asm),
                          os.path.join(ROOT, "suchtree_amd", "csrc", "launch_canopy.hip")], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    bodies, name = {}, None
    for line in asm.read_text().splitlines():
        m = re.match(r"(_ZN2st\d+k_canopy_ilp\w+):", line)
        if m:
            name = m.group(1)
            bodies[name] = []
        elif line.startswith(".Lfunc_end"):
            name = None
        elif name:
            bodies[name].append(line.split(";")[0].strip())
    return bodies


def _count(body, mnemonic):
    """(with nt, without) among the instructions of that mnemonic"""
    hits = [l for l in body if re.match(mnemonic + r"\s", l)]
    hinted = sum(1 for l in hits if re.search(r"\bnt\b", l))
    return hinted, len(hits) - hinted


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_heap_kernel_streams_carry_the_hint_and_line_loads_do_not(kernel_bodies):
    heap = {k: v for k, v in kernel_bodies.items() if "k_canopy_ilp_heap" in k}
    assert len(heap) == 2, sorted(heap)
    body = next(v for k, v in heap.items() if "9SrcContigE" in k)
    hinted, plain = _count(body, "global_load_dwordx4")
    # the pair load in its hinted form; image staging, the plain pair load and the four line loads of either copy of the loop without
    assert hinted == 1 and plain >= 10, (hinted, plain)
    hinted, plain = _count(body, "global_store_dwordx2")      # float64 distances
    assert hinted >= 1 and plain >= 1, (hinted, plain)
    hinted, plain = _count(body, "global_store_dword")        # float32 distances, int32 ids, the packed ids' dwords
    assert hinted >= 3 and plain >= 3, (hinted, plain)
    for mnemonic in ("global_store_byte", "global_store_short"):      # (the hint must not have split a store)
        assert _count(body, mnemonic) == (0, 0), mnemonic


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_general_table_kernels_keep_the_hinted_pair_load(kernel_bodies):
    """k_canopy_ilp<..., SrcContig / SrcContig32, ...>: a hinted 16-byte / 8-byte pair load beside the plain one, and plain stores;
    the heap-line kernel of the int32 source keeps its plain loop alone."""
    plain_kernels = {k: v for k, v in kernel_bodies.items() if "k_canopy_ilpI" in k}
    assert plain_kernels
    for name, body in plain_kernels.items():
        mnemonic = "global_load_dwordx4" if "9SrcContigE" in name else "global_load_dwordx2"
        hinted, plain = _count(body, mnemonic)
        assert hinted == 1 and plain >= 1, (name, hinted, plain)
        for store in ("global_store_dword", "global_store_dwordx2"):
            assert _count(body, store)[0] == 0, (name, store)
    body32 = next(v for k, v in kernel_bodies.items() if "k_canopy_ilp_heap" in k and "11SrcContig32E" in k)
    assert not [l for l in body32 if re.search(r"\bnt\b", l)]
