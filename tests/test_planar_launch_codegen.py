"""Guards what the SoftPendulum launch does AROUND its substep loop: a planar rod in range writes no
scratch on its way to the loop.  Until the planar launch rework the kernel parked the addresses of the
rows only its cold paths store (NaN fill, the launch that only constrains) — twelve dwordx2 per lane,
24 MiB of dirty spill lines per 4096-env launch that nothing ever read back, half of what the launch
wrote to HBM.  Those paths now go through the out-of-line cold call and the kernel
re-derives its store addresses behind the loop."""
import re
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "gym_softrobot_amd" / "csrc"
KERNEL = "fast_kernelILj15ELi1ELi1E"          # <SOFTPENDULUM, SOFTPENDULUM, EPL = 1>
PARENT_SCRATCH = 988                          # private_segment_fixed_size before the rework


@pytest.fixture(scope="module")
def isa_text(tmp_path_factory):
    """The gfx950 ISA of the whole library (one hipcc -S run for the module)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("isa") / "capi.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only",
                    "-o", str(asm), str(CSRC / "softrod_capi.hip")], check=True, timeout=900,
                   stderr=subprocess.DEVNULL)
    return asm.read_text()


@pytest.fixture(scope="module")
def walked(isa_text):
    sys.path.insert(0, str(ROOT / "tools"))
    import hot_path_isa

    ins, labels = hot_path_isa.function_body(isa_text, KERNEL)
    return hot_path_isa, ins, labels


def _loop_header(hot_path_isa, ins, labels):
    """Index of the hot loop's header: the first instruction of the walked substep."""
    path = hot_path_isa.hot_path(ins, labels)
    heads = [i for i in sorted(set(labels.values())) if ins[i:i + 8] == path[:8]]
    assert heads, "the hot loop's header was not found among the kernel's labels"
    return heads[0]


def test_no_scratch_store_on_the_way_to_the_hot_loop(walked):
    hot_path_isa, ins, labels = walked
    calls = [i for i, x in enumerate(ins) if "s_swappc" in x]
    assert len(calls) == 1, "one out-of-line call (the cold path) is expected"
    bounds = sorted(set(labels.values()))
    lo = max(b for b in bounds if b <= calls[0])
    hi = min([b for b in bounds if b > calls[0]] + [len(ins)])
    header = _loop_header(hot_path_isa, ins, labels)
    before = [i for i, x in enumerate(ins[:header]) if x.startswith("scratch_store") and not lo <= i < hi]
    assert not before, f"{len(before)} scratch stores before the hot loop outside the cold-call block: {before}"


def test_hot_path_is_unmoved(walked):
    hot_path_isa, ins, labels = walked
    path = hot_path_isa.hot_path(ins, labels)
    valu = [x for x in path if x.startswith("v_")]
    assert len(valu) <= 99, f"planar substep grew to {len(valu)} VALU instructions"
    # no memory instruction of any kind: vector (global / flat / buffer / scratch), LDS, or scalar loads
    memory = ("scratch", "global", "buffer", "flat", "ds_", "s_load", "s_buffer_load")
    assert not [x for x in path if x.startswith(memory)]
    assert not [x for x in valu if x.startswith("v_mov_b64")], "register copies inside the planar substep"


def test_private_segment_not_above_the_parents(isa_text):
    for m in re.finditer(r"- \.agpr_count:.*?\.wavefront_size:\s+\d+", isa_text, re.S):
        blk = m.group(0)
        if KERNEL in re.search(r"\.name:\s+(\S+)", blk).group(1):
            size = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
            assert size <= PARENT_SCRATCH, f"private_segment_fixed_size grew to {size}"
            return
    raise AssertionError(f"kernel {KERNEL} not found in the metadata")
