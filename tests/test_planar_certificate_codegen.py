"""Guards what planar certificates buy (csrc/softrod_planar.hpp): on its way to the substep loop a SoftPendulum rod
that holds a certificate loads the seven rows of the planar state and its per-rod scalars and nothing else — the
eleven rows and five boundary-condition targets of the planarity proof sit behind one wave-uniform branch — and the
loop itself is the 98 VALU instructions it was.  Same cross-compile and the same walker (tools/hot_path_isa.py) as
tests/test_planar_launch_codegen.py."""
import heapq
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "gym_softrobot_amd" / "csrc"
KERNEL = "fast_kernelILj15ELi1ELi1E"          # <SOFTPENDULUM, SOFTPENDULUM, EPL = 1>
STATE_ROWS = 7                                # x, y, v_x, v_y, d3_x, d3_y, omega_2
# float64 values per rod that are no state row: the three in-plane BC targets, the clock, the clock table's entry
ROD_SCALARS = 3 + 1 + 1
PROOF_LOADS = 11 + 5                          # the other rows of the 18 and the other BC targets the proof compares


@pytest.fixture(scope="module")
def kernel():
    """The instructions and labels of the kernel, from one hipcc -S run of the whole library."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    sys.path.insert(0, str(ROOT / "tools"))
    import hot_path_isa

    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        asm = Path(tmp) / "capi.s"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                        "-o", str(asm), str(CSRC / "softrod_capi.hip")], check=True, timeout=900,
                       stderr=subprocess.DEVNULL)
        ins, labels = hot_path_isa.function_body(asm.read_text(), KERNEL)
    return hot_path_isa, ins, labels


def _loop_header(hot_path_isa, ins, labels):
    path = hot_path_isa.hot_path(ins, labels)
    heads = [i for i in sorted(set(labels.values())) if ins[i:i + 8] == path[:8]]
    assert heads, "the hot loop's header was not found among the kernel's labels"
    return heads[0]


def _successors(ins, labels, i):
    m = re.match(r"(s_cbranch_\w+|s_branch)\s+(\.LBB\d+_\d+)", ins[i])
    if ins[i].startswith("s_endpgm"):
        return []
    if m and m.group(1) == "s_branch":
        return [labels[m.group(2)]]
    if m:
        return [labels[m.group(2)], i + 1]
    return [i + 1] if i + 1 < len(ins) else []


def _is_load(x):
    return x.startswith(("global_load_dwordx2", "flat_load_dwordx2", "buffer_load_dwordx2"))


def _fewest_loads(ins, labels, target, through=None):
    """The fewest float64 loads any path from the kernel's entry to `target` executes (through instruction `through`,
    if given): Dijkstra over the instructions, an edge costing 1 where it leaves a load."""
    def run(src, dst):
        dist = {src: 0}
        heap = [(0, src)]
        while heap:
            d, i = heapq.heappop(heap)
            if i == dst:
                return d
            if d > dist.get(i, 1 << 30):
                continue
            for j in _successors(ins, labels, i):
                nd = d + (1 if _is_load(ins[i]) else 0)
                if nd < dist.get(j, 1 << 30):
                    dist[j] = nd
                    heapq.heappush(heap, (nd, j))
        raise AssertionError(f"instruction {dst} is not reachable from {src}")
    return run(0, target) if through is None else run(0, through) + run(through, target)


def test_a_certified_rod_loads_the_planar_state_only(kernel):
    hot_path_isa, ins, labels = kernel
    header = _loop_header(hot_path_isa, ins, labels)
    certified = _fewest_loads(ins, labels, header)
    assert certified <= STATE_ROWS + ROD_SCALARS, f"{certified} float64 loads on the certified rod's way to the loop"
    assert certified >= STATE_ROWS                   # (the walk did find the loads)
    # the proof's loads are behind a branch of their own: the way to the loop through the block that holds the most
    # loads ahead of the loop (outside the cold call's) costs exactly the proof's loads more
    calls = [i for i, x in enumerate(ins) if "s_swappc" in x]
    bounds = sorted(set(labels.values()) | {0, len(ins)} | {i + 1 for i, x in enumerate(ins) if re.match(r"s_c?branch", x)})
    blocks = [(a, b) for a, b in zip(bounds, bounds[1:]) if b <= header and not a <= calls[0] < b]
    a, b = max(blocks, key=lambda ab: sum(_is_load(x) for x in ins[ab[0]:ab[1]]))
    assert sum(_is_load(x) for x in ins[a:b]) == PROOF_LOADS, "the proof's loads are not one block of the kernel"
    assert _fewest_loads(ins, labels, header, through=a) == certified + PROOF_LOADS
    # the two bytes (the rod's certificate, the switch) are asked for ahead of every row, behind the auto-reset
    # pass's skip flag
    first_row = next(i for i, x in enumerate(ins) if _is_load(x))
    assert sum(x.startswith("global_load_ubyte") for x in ins[:first_row]) == 3


def test_the_substep_is_the_98_instructions_it_was(kernel):
    hot_path_isa, ins, labels = kernel
    path = hot_path_isa.hot_path(ins, labels)
    valu = [x for x in path if x.startswith("v_")]
    assert len(valu) == 98, f"the planar substep has {len(valu)} VALU instructions"
    memory = ("scratch", "global", "buffer", "flat", "ds_", "s_load", "s_buffer_load")
    assert not [x for x in path if x.startswith(memory)]
