"""CPU tier: the prologue of the decode matvec and of the fused decode attention runs UNDER the first weight tile / KV page request,
read off the gfx950 code objects inside the built libaha_hip.so (extracted the way tests/test_attn_decode_chain_cpu.py does).

Returns are in order within a wave, so "under" means: every wait on a vector-memory return between the kernel's first non-temporal
(`nt`) load -- the first weight tile of the matvec, the unit's first K/V page of the attention; nothing else in these kernels is loaded
`nt` -- and the barrier that ends the prologue is a COUNTED wait that leaves that whole request in flight: `s_waitcnt vmcnt(N)` with
N >= the number of `nt` loads issued so far (8 for the one-row kernels, 16 for gate+up and the lm_head, 32 for a K/V page).  The
compiler only counts what is outstanding on every path, which is why these kernels request nothing under a run-time condition there
(aha_amd/csrc/gemv_body.h, attn_decode_body.h).

Scope: the non-traced straight-line matvec instantiations of the four decode plans -- <R, U, EPI> = <1, 8, store> (qkv), <1, 8, residual>
(o_proj, down), <2, 4, silu_mul> (gate+up), <4, 4, logits> (lm_head), each without (PRO = 1) and with (PRO = 2) norm weights -- and the two
fused decode attention kernels.

Which path is walked: all of them.  The scan takes the program text in order from the first `nt` load to the prologue's last barrier
(the second `s_barrier` where the RMSNorm's reduction adds one, the first otherwise).  The compiler lays the prologue out in source order
and the only branches in that stretch are forward skips around LDS writes (`if (v < nvec) stage(..)`, `if (p_have) norm_rope(..)`), so a
decode launch executes a subsequence of exactly these instructions, whatever its shape; the scan asserts that no branch there goes
backwards.  The attention's rounds beyond the second (g >= 8) load under a condition and sit behind that barrier on purpose.
"""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
# (R, U, EPI): nt loads of the first weight tile = R * U * (2 for silu_mul)
PLANS = {(1, 8, 0): 8, (1, 8, 1): 8, (2, 4, 2): 16, (4, 4, 3): 16}
MATVECS = [(r, u, e, pro) for (r, u, e) in PLANS for pro in (1, 2)]
ATTN = ("attn_decode_fused_kernelE", "attn_decode_fused_table_kernelE")
PAGE_LOADS = 32


def gemv_tag(r, u, e, pro):
    return f"gemv_kernelILi{r}ELi{u}ELi{e}ELb1ELb0ELi{pro}EE"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """{tag: (vgpr_count, program text as a list of instructions)} of the kernels in scope."""
    if not (os.path.exists(f"{LLVM}/llvm-objdump") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm llvm tools not found")
    from aha_amd import build
    build.build()
    d = tmp_path_factory.mktemp("codeobj")
    shutil.copy(os.path.join(ROOT, "aha_amd", "csrc", "libaha_hip.so"), d / "lib.so")
    subprocess.run([f"{LLVM}/llvm-objdump", "--offloading", "lib.so"], cwd=d, capture_output=True, check=True)   # writes lib.so.N.<target>
    tags = [gemv_tag(*k) for k in MATVECS] + list(ATTN)
    out = {}
    for o in sorted(glob.glob(str(d / "lib.so.*gfx950"))):
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", o], capture_output=True, text=True, check=True).stdout
        if not any(t in notes for t in tags):
            continue
        vgprs = {}
        for item in re.split(r"\n  - ", notes[notes.index("amdhsa.kernels:"):])[1:]:
            name = re.search(r"^\s*\.name:\s+(\S+)", item, re.M)
            count = re.search(r"^\s*\.vgpr_count:\s+(\d+)", item, re.M)
            if name and count:
                vgprs[name.group(1)] = int(count.group(1))
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", o], capture_output=True, text=True, check=True).stdout
        cur = None
        for line in dis.splitlines():
            m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
            if m:
                hit = [t for t in tags if t in m.group(1)]
                cur = hit[0] if hit else None
                if cur:
                    assert cur not in out, f"two kernels match {cur}"
                    out[cur] = (vgprs[m.group(1)], [])
                continue
            t = line.strip().split("//")[0].strip()
            if cur and t:
                out[cur][1].append(t)
    assert sorted(out) == sorted(tags), sorted(set(tags) - set(out))
    return out


def is_nt_load(t):
    return t.startswith("global_load_dwordx4") and t.split()[-1] == "nt"


def vm_waits(text):
    """(index, N) of every wait with a vmcnt field."""
    out = []
    for i, t in enumerate(text):
        m = re.search(r"vmcnt\((\d+)\)", t) if t.startswith("s_waitcnt") else None
        if m:
            out.append((i, int(m.group(1))))
    return out


def prologue_stretch(text, barriers):
    """Indices [first nt load, the `barriers`-th s_barrier behind it]."""
    first = next(i for i, t in enumerate(text) if is_nt_load(t))
    ends = [i for i, t in enumerate(text) if t.startswith("s_barrier") and i > first]
    assert len(ends) >= barriers
    return first, ends[barriers - 1]


def check_counted(text, barriers, tile_loads):
    first, end = prologue_stretch(text, barriers)
    issued = 0
    seen = []
    for i in range(first, end):
        t = text[i]
        if is_nt_load(t):
            issued += 1
        if t.startswith("s_cbranch") or t.startswith("s_branch"):
            assert int(t.split()[1]) < 0x8000, f"backward branch in the prologue: {t}"
        m = re.search(r"vmcnt\((\d+)\)", t) if t.startswith("s_waitcnt") else None
        if m:
            seen.append(int(m.group(1)))
            assert int(m.group(1)) >= issued, f"`{t}` with {issued} nt loads issued: the wait drains the first request"
    assert issued == tile_loads, (issued, tile_loads)   # the whole first request, and only it, is in flight in front of that barrier
    return seen


@pytest.mark.parametrize("r,u,e,pro", MATVECS)
def test_matvec_prologue_waits_leave_the_first_weight_tile_in_flight(kernels, r, u, e, pro):
    _, text = kernels[gemv_tag(r, u, e, pro)]
    seen = check_counted(text, 2 if pro == 2 else 1, PLANS[(r, u, e)])
    assert seen, "no wait at all in front of the barrier: the scan does not see the staging"
    first = next(i for i, t in enumerate(text) if is_nt_load(t))
    assert [n for i, n in vm_waits(text) if i < first] == [], "a vector-memory wait in front of the first weight request"


@pytest.mark.parametrize("r,u,e,pro", MATVECS)
def test_matvec_register_count(kernels, r, u, e, pro):
    """Not above the kernels this form replaces (127 for the 8-load tiles, 166 gate+up, 170 lm_head): the blocks per CU stay what they were."""
    vgprs, _ = kernels[gemv_tag(r, u, e, pro)]
    assert vgprs <= {8: 127, 16: 166 if e == 2 else 170}[PLANS[(r, u, e)]], vgprs


def test_attention_prologue_waits_leave_the_page_in_flight(kernels):
    _, linear = kernels[ATTN[0]]
    seen = check_counted(linear, 1, PAGE_LOADS)
    assert seen, "no wait at all in front of the barrier: the scan does not see the norm/rope"
    first = next(i for i, t in enumerate(linear) if is_nt_load(t))
    assert [n for i, n in vm_waits(linear) if i < first] == [], "a vector-memory wait in front of the first K/V request"
    # The table form has to wait for its page pointers in front of the page request (tests/test_attn_decode_chain_cpu.py holds it to
    # that), and that wait, behind the prologue's inputs in issue order, covers them: behind the request nothing is left to wait for.
    _, table = kernels[ATTN[1]]
    check_counted(table, 1, PAGE_LOADS)


def test_the_scan_sees_a_draining_wait():
    """The general FAST form (PRO = 0) still loads under conditions: were it scanned, it would fail.  Checked on a literal excerpt."""
    text = ["global_load_dwordx4 v[0:3], v[4:5], off", "global_load_dwordx4 v[6:9], v[4:5], off nt", "s_waitcnt vmcnt(0)", "s_barrier"]
    with pytest.raises(AssertionError):
        check_counted(text, 1, 1)
