"""What the compiler made of the early request for the observed-pixel records (post_seq.hpp stage_and_obs), read off the assembly
of the unit that holds `payne_post_kernel<12, true, true>` (the C2 likelihood kernel).  No GPU needed: hipcc cross-compiles."""
import os
import re
import subprocess

import pytest


@pytest.fixture(scope="module")
def c2_kernel(tmp_path_factory):
    from thepayne_amd import build
    asm = tmp_path_factory.mktemp("asm") / "k_post_lean.s"
    cmd = [build._hipcc()] + [f for f in build.HIPCC_FLAGS if f != "-fPIC"] + ["-I", os.path.join(build.ROOT, "include"), "-S", "--cuda-device-only",
                                                                           os.path.join(build.CSRC, "k_post_lean.hip"), "-o", str(asm)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = asm.read_text()
    m = re.search(r"^_Z17payne_post_kernelILi12ELb1ELb1EE\w*:.*?s_endpgm", text, re.S | re.M)
    assert m
    summary = re.search(r"^_Z17payne_post_kernelILi12ELb1ELb1EE\w*:.*?; NumVgprs: (\d+).*?; ScratchSize: (\d+).*?; Occupancy: (\d+)", text, re.S | re.M)
    meta = re.search(r"\.name:\s+_Z17payne_post_kernelILi12ELb1ELb1EE\w*.*?\.vgpr_spill_count:\s+(\d+)", text, re.S)
    assert summary and meta
    return m.group(0).splitlines(), tuple(int(x) for x in summary.groups()), int(meta.group(1))


def _code(line):
    return line.split(";")[0]


def _records_block(body):
    """Index of the first and the last request of the block of eight records that stage_and_obs issues: eight 16-byte loads without
    a barrier among them, the first off the table's base in scalar registers, FOLLOWED by the stage's nine LDS-only barriers (4
    forward passes, the Gaussian product, 4 inverse passes) with no vector-memory load among them."""
    loads = [i for i, l in enumerate(body) if "global_load_dwordx4" in _code(l)]
    barriers = [i for i, l in enumerate(body) if re.match(r"\s*s_barrier\b", _code(l))]
    found = []
    for n in range(len(loads) - 7):
        first, last = loads[n], loads[n + 7]
        if any(first < b < last for b in barriers):
            continue
        nxt = [b for b in barriers if b > last][:9]
        if len(nxt) < 9:
            continue
        if any("global_load" in _code(l) or "buffer_load" in _code(l) or "flat_load" in _code(l) for l in body[last + 1:nxt[-1]]):
            continue
        found.append((first, last, nxt))
    assert len(found) == 1, [(f, l) for f, l, _ in found]
    return found[0]


def test_records_are_requested_ahead_of_the_forward_transform_and_never_waited_for_before_the_loop(c2_kernel):
    body, _, _ = c2_kernel
    first, last, barriers = _records_block(body)
    # the nine barriers behind the request wait for LDS traffic only: `s_waitcnt lgkmcnt(0)` right in front of each, and from the
    # request to the last of them nothing waits on the vector-memory counter at all
    for b in barriers:
        assert re.match(r"\s*s_waitcnt lgkmcnt\(0\)\s*$", _code(body[b - 1])), (b, body[b - 1])
    stage = body[last + 1:barriers[-1] + 1]
    waits = [l for l in stage if "s_waitcnt" in _code(l) and "vmcnt" in _code(l)]
    assert not waits, waits
    assert not any("s_swappc" in _code(l) or "s_setpc" in _code(l) for l in stage)            # (a call would wait for every load)
    # behind the last barrier the loop takes the records one by one, oldest first: the first wait on the counter lets seven requests
    # stay in flight, and no `vmcnt(0)` comes before it
    after = [_code(l) for l in body[barriers[-1] + 1:] if "s_waitcnt" in _code(l) and "vmcnt" in _code(l)]
    assert after and re.search(r"vmcnt\(7\)", after[0]), after[:3]
    # ... which are the requests in the order of the loop: record 0 (no offset from the table's base, which sits in scalar
    # registers) first
    reqs = [_code(l) for l in body[first:last + 1] if "global_load_dwordx4" in _code(l)]
    assert len(reqs) == 8 and re.search(r"s\[\d+:\d+\]\s*$", reqs[0].rstrip()), reqs
    dest = [int(re.search(r"global_load_dwordx4 v\[(\d+):", r).group(1)) for r in reqs]
    use = []                                                  # the order in which the loop first reads each record's position
    for l in body[barriers[-1] + 1:barriers[-1] + 400]:
        m = re.match(r"\s*v_fma_f64 v\[\d+:\d+\], v\[(\d+):\d+\],", _code(l))
        if m and int(m.group(1)) in dest and int(m.group(1)) not in use:
            use.append(int(m.group(1)))
    assert use == dest, (use, dest)


def test_the_block_of_records_costs_no_occupancy_and_no_scratch(c2_kernel):
    """Thirty-two more registers live across nine barrier intervals: the kernel still fits 128 vector registers (two workgroups per
    compute unit), spills none of them, and no instruction of it touches scratch memory (the 24 bytes of its summary are the frame
    its out-of-line walk step may use)."""
    body, (vgprs, scratch, occ), spilled = c2_kernel
    assert vgprs <= 128 and occ >= 4, (vgprs, occ)
    assert spilled == 0
    assert scratch <= 24, scratch
    assert not [l for l in body if l.startswith("\t") and "scratch_" in _code(l)]
