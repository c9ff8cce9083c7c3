"""tests/asm_hazards.py: the waitcnt dataflow checker on hand-written disassembly, on compiled controls, and on every kernel that ships.
CPU only: the device code is cross-compiled for gfx950 and disassembled here, nothing is launched."""
from __future__ import annotations

import os
import subprocess
import textwrap
from concurrent.futures import ProcessPoolExecutor

import pytest

from tests import asm_hazards as A
from vtamiq_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))


def _asm(body: str) -> str:
    """A one-kernel llvm-objdump listing: 'Ln:' lines become <Ln> labels, every other line an instruction at the next address."""
    lines, addr = ["0000000000001000 <k>:"], 0x1000
    for raw in textwrap.dedent(body).strip().splitlines():
        raw = raw.strip()
        if not raw:
            continue
        if raw.endswith(":"):
            lines += ["", f"{addr:016x} <{raw[:-1]}>:"]
        else:
            lines.append(f"\t{raw:<58s} // {addr:012X}: 00000000")
            addr += 4
    return "\n".join(lines) + "\n"


def _findings(body: str):
    return A.analyze_text(_asm(body))["k"].findings


def _one(body: str, insn: str, load: str, counter: str, wait: str):
    f = _findings(body)
    assert [(x.insn, x.load, x.counter, x.wait) for x in f] == [(insn, load, counter, wait)], [str(x) for x in f]


# ---- synthetic disassembly ------------------------------------------------------------------------------------------------------

def test_read_before_wait_is_flagged():
    _one("""
        global_load_dword v1, v[2:3], off
        v_add_f32_e32 v4, v1, v1
        s_waitcnt vmcnt(0)
        s_endpgm
    """, "v_add_f32_e32 v4, v1, v1", "global_load_dword v1, v[2:3], off", A.VM, "vmcnt(0)")


def test_read_behind_covering_wait_is_clean():
    assert _findings("""
        global_load_dword v1, v[2:3], off
        global_load_dword v5, v[2:3], off offset:4
        s_waitcnt vmcnt(1)
        v_add_f32_e32 v4, v1, v1
        s_waitcnt vmcnt(0)
        v_add_f32_e32 v6, v5, v5
        s_endpgm
    """) == []


def test_stores_and_lds_dma_take_vm_slots():
    # younger store and LDS-DMA: vmcnt(2) retires the load (clean only if both are counted)
    assert _findings("""
        global_load_dword v1, v[2:3], off
        global_store_dword v[2:3], v7, off
        global_load_lds_dwordx4 v[8:9], off
        s_waitcnt vmcnt(2)
        v_add_f32_e32 v4, v1, v1
        s_endpgm
    """) == []
    # miscount: the store the wait counted on is OLDER than the load, so vmcnt(1) leaves the load in flight
    _one("""
        global_store_dword v[2:3], v7, off
        global_load_dword v1, v[2:3], off
        s_waitcnt vmcnt(1)
        v_add_f32_e32 v4, v1, v1
        s_endpgm
    """, "v_add_f32_e32 v4, v1, v1", "global_load_dword v1, v[2:3], off", A.VM, "vmcnt(0)")


def test_write_after_write_on_the_same_counter_is_clean():
    assert _findings("""
        global_load_dword v1, v[2:3], off
        global_load_dword v1, v[2:3], off offset:4
        ds_read_b32 v5, v6
        ds_read_b64 v[4:5], v6 offset:8
        s_waitcnt vmcnt(0) lgkmcnt(0)
        v_add_f32_e32 v7, v1, v5
        s_endpgm
    """) == []


def test_vm_write_over_pending_lds_read_is_flagged():
    _one("""
        ds_read_b32 v1, v2
        global_load_dword v1, v[4:5], off
        s_waitcnt vmcnt(0) lgkmcnt(0)
        s_endpgm
    """, "global_load_dword v1, v[4:5], off", "ds_read_b32 v1, v2", A.LDS, "lgkmcnt(0)")


def test_smem_is_retired_only_by_lgkmcnt0():
    _one("""
        s_load_dword s4, s[0:1], 0x0
        ds_read_b32 v1, v2
        s_waitcnt lgkmcnt(1)
        s_add_i32 s5, s4, 1
        s_waitcnt lgkmcnt(0)
        s_add_i32 s6, s4, 1
        s_endpgm
    """, "s_add_i32 s5, s4, 1", "s_load_dword s4, s[0:1], 0x0", A.SMEM, "lgkmcnt(0)")


LOOP = """
    s_mov_b32 s2, 4
    L0:
    v_add_f32_e32 v8, v1, v8
    global_load_dword v1, v[2:3], off
    s_sub_i32 s2, s2, 1
    s_cmp_lg_u32 s2, 0
    {wait}
    s_cbranch_scc1 L0
    s_waitcnt vmcnt(0)
    s_endpgm
"""


def test_load_pending_across_back_edge_is_flagged():
    _one(LOOP.format(wait=""), "v_add_f32_e32 v8, v1, v8", "global_load_dword v1, v[2:3], off", A.VM, "vmcnt(0)")


def test_loop_with_wait_is_clean():
    assert _findings(LOOP.format(wait="s_waitcnt vmcnt(0)")) == []


def test_join_with_one_path_waited_is_flagged():
    _one("""
        global_load_dword v1, v[2:3], off
        s_cbranch_scc1 L1
        s_waitcnt vmcnt(0)
        L1:
        v_add_f32_e32 v4, v1, v1
        s_endpgm
    """, "v_add_f32_e32 v4, v1, v1", "global_load_dword v1, v[2:3], off", A.VM, "vmcnt(0)")


def test_flag_lowered_if_else_chain_is_clean():
    # hipcc's lowering of `if (c) wait(0); else wait(1);` through a flag in s[8:9]: no path skips both waits
    assert _findings("""
        global_load_dword v1, v[2:3], off
        global_store_dword v[2:3], v7, off
        s_mov_b64 s[8:9], -1
        s_and_b64 vcc, exec, s[6:7]
        s_cbranch_vccz L0
        s_waitcnt vmcnt(0)
        s_mov_b64 s[8:9], 0
        L0:
        s_andn2_b64 vcc, exec, s[8:9]
        s_cbranch_vccnz L1
        s_waitcnt vmcnt(1)
        L1:
        v_add_f32_e32 v4, v1, v1
        s_endpgm
    """) == []


@pytest.mark.parametrize("write", ["v_cmp_gt_u32_e64 s[8:9], v5, v6\n s_and_b64 vcc, exec, s[8:9]",
                                   "s_and_b64 vcc, exec, s[8:9]\n v_cmp_gt_u32_e32 vcc, v5, v6",
                                   "v_readlane_b32 s8, v5, 0\n s_and_b64 vcc, exec, s[8:9]"])
def test_valu_writes_clear_known_flags(write):
    # s[8:9] / vcc are rewritten by a VALU op after the constant: both branch edges stay feasible, the hazard is reported
    body = "global_load_dword v1, v[2:3], off\n s_mov_b64 s[8:9], 0\n" + write + """
        s_cbranch_vccz L0
        v_add_f32_e32 v4, v1, v1
        L0:
        s_waitcnt vmcnt(0)
        s_endpgm"""
    _one(body, "v_add_f32_e32 v4, v1, v1", "global_load_dword v1, v[2:3], off", A.VM, "vmcnt(0)")


@pytest.mark.parametrize("insn", ["global_load_dwordx9 v[0:8], v[2:3], off", "flat_load_dword v1, v[2:3]", "ds_frobnicate_b32 v1, v2",
                                  "buffer_load_dword v1, v2, s[0:3], 0 offen lds"])
def test_unknown_memory_mnemonic_is_an_error(insn):
    with pytest.raises(A.AsmHazardError):
        _findings(insn + "\ns_endpgm")


@pytest.mark.parametrize("insn", ["s_setpc_b64 s[0:1]", "s_swappc_b64 s[30:31], s[0:1]", "s_cbranch_execz s[0:1]"])
def test_indirect_control_flow_is_an_error(insn):
    with pytest.raises(A.AsmHazardError):
        _findings(insn + "\ns_endpgm")


# ---- compiled controls ------------------------------------------------------------------------------------------------------------

def test_compiled_controls(tmp_path):
    obj = str(tmp_path / "asm_hazard_controls.o")
    subprocess.run([build._hipcc()] + build.FLAGS + ["-c", os.path.join(HERE, "asm_hazard_controls.hip"), "-o", obj], check=True)
    rep = A.analyze_object(obj, str(tmp_path))
    assert rep.device and set(rep.kernel_symbols) == set(rep.kernels)
    got = {k.name: [(f.insn.split()[0], f.load.split()[0], f.counter, f.wait) for f in k.findings] for k in rep.kernels.values()}
    assert got == {
        "ctl_a": [("v_mov_b32_e32", "global_load_dword", A.VM, "vmcnt(0)")],
        "ctl_b": [("v_mov_b32_e32", "global_load_dword", A.VM, "vmcnt(0)")],
        "ctl_c": [("v_mov_b32_e32", "ds_read_b32", A.LDS, "lgkmcnt(0)")],
        "ctl_a_clean": [], "ctl_b_clean": [], "ctl_c_clean": [],
    }, got
    # ctl_b: the flagged read is of the YOUNGER load (offset:4); ctl_c: of the younger ds_read (offset:256)
    b = rep.kernels["ctl_b"].findings[0]
    c = rep.kernels["ctl_c"].findings[0]
    assert b.load.endswith("offset:4") and b.regs == tuple(b.load.split()[1].rstrip(",").split(","))
    assert c.load.endswith("offset:256") and c.regs == (c.load.split()[1].rstrip(","),)


# ---- the shipped kernels ------------------------------------------------------------------------------------------------------------

def _analyze_all():
    objs = [o for objdir, lib in A.LIBRARIES.values() for o in A.shipped_objects(objdir, lib)]
    with ProcessPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return dict(zip(objs, ex.map(A.analyze_object, objs)))


@pytest.fixture(scope="module")
def shipped():
    return _analyze_all()


# attention_sw_kernel findings argued infeasible from the source, one entry per (kernel, instruction, pending load), each with its
# reason (tests/golden/asm_hazards_baseline.json).  Anything else -- in attention.hip or elsewhere -- fails; so does a baseline entry
# that no longer occurs (the baseline must be re-triaged when the kernel changes).
def _baseline():
    import json
    with open(os.path.join(HERE, "golden", "asm_hazards_baseline.json")) as f:
        data = json.load(f)
    return {(e["kernel"], e["insn"], e["load"]): data["reasons"][e["reason"]] for e in data["findings"]}


@pytest.mark.parametrize("source", build.SOURCES)
def test_shipped_kernels_have_no_findings(shipped, source):
    base = _baseline()
    seen = set()
    for rep in shipped.values():
        if rep.source != source:
            continue
        bad = []
        for k in rep.kernels.values():
            for f in k.findings:
                key = (k.name, f.insn, f.load)
                (seen.add(key) if key in base else bad.append(str(f)))
        assert not bad, f"{rep.path}: {len(bad)} findings\n" + "\n".join(bad[:20])
    stale = [k for k in base if source == "attention.hip" and k not in seen]
    assert not stale, f"baseline entries that no longer occur: {stale[:5]}"


def test_every_kernel_is_analysed_in_both_builds(shipped):
    assert len(shipped) == 2 * len(build.SOURCES)
    for rep in shipped.values():
        if not rep.device:                      # host-only translation unit: it must define no kernel
            with open(os.path.join(build.CSRC, rep.source)) as f:
                assert "__global__" not in f.read(), rep.path
            continue
        assert rep.kernel_symbols and set(rep.kernels) == set(rep.kernel_symbols), rep.path
        for k in rep.kernels.values():
            assert k.instructions > 0 and (k.vm_ops + k.lgkm_ops) > 0, (rep.path, k.demangled)


@pytest.mark.parametrize("objdir", ["_obj", "_obj_fp8"])
def test_asm_sync_sites_are_covered(shipped, objdir):
    reps = [r for o, r in shipped.items() if os.path.basename(os.path.dirname(o)) == objdir]

    def kernels(sub):
        ks = [k for r in reps for k in r.kernels.values() if sub in k.demangled]
        assert ks, sub
        return ks

    for k in kernels("attention_sw_kernel"):           # asm Q loads (dwordx4) and the Q L2 prefetch (dword)
        assert k.mnemonics["global_load_dwordx4"] > 0 and k.mnemonics["global_load_dword"] > 0, k.demangled
        assert k.mnemonics["ds_read_b64_tr_b16"] > 0, k.demangled
    for k in kernels("gemm_rowln"):
        assert k.mnemonics["ds_read_b128"] > 0, k.demangled
    for k in kernels("gemm_pp2_kernel"):
        assert k.mnemonics["global_load_lds_dwordx4"] > 0, k.demangled
