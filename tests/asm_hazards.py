"""Static check of the shipped device code: no register is read, copied or overwritten while a memory op that writes it is in flight.

Several kernels issue loads from inline asm and retire them with hand-counted `s_waitcnt` (attention.hip: the Q loads and the Q L2
prefetch, the counted `lgkmcnt` ties of the fragment reads; gemm_rowln.hip: `ds_read_b128` batches; gemm.hip: LDS-DMA under counted
`vmcnt`).  The compiler's waitcnt pass does not see inside asm, so those kernels are correct only while the compiler never reads or
re-allocates an asm load's destination before the asm wait that retires it, never places a memory op of its own between an asm load
and its counted wait, and never hoists a reader above such a wait.  This module checks that, exactly, on the code objects that ship:

  * input: every object of vtamiq_amd/csrc/_obj and _obj_fp8 (the ones build.py links); the gfx950 code object is taken from the
    object's `.hip_fatbin` section, unbundled with `clang-offload-bundler --unbundle --type=o` and disassembled with
    `llvm-objdump -d --symbolize-operands` (both from ROCm's llvm/bin; a missing tool is an error);
  * CFG per kernel symbol: blocks cut at `<Ln>:` labels and after branches; `s_cbranch_*` has two successors, `s_branch` one,
    `s_endpgm` none.  Indirect control flow or calls raise `AsmHazardError` (nothing is guessed);
  * abstract state: one ordered list of pending ops per counter, youngest last, each position holding the ops (and the registers
    they will write) that may sit there.  vmcnt is in order (as LLVM's SIInsertWaitcnts assumes for gfx9) and counts every
    global_ / buffer_ / scratch_ op: loads, stores, atomics, LDS-DMA (no VGPR destination, still a slot), buffer_wbl2 / buffer_inv.
    LDS ops are in order among themselves on lgkmcnt; SMEM loads (`s_load*` / `s_buffer_load*`, and `s_memtime` /
    `s_memrealtime`) return out of order and are retired only by lgkmcnt(0).  flat_ ops, and any global_ / buffer_ / scratch_ /
    flat_ / ds_ mnemonic the tables below do not classify, raise `AsmHazardError`;
  * transfer: `s_waitcnt vmcnt(N)` keeps the N youngest VM positions, `lgkmcnt(N)` the N youngest LDS positions (SMEM only goes at
    N = 0); an op appends a position; a list longer than the hardware field (vmcnt 63, lgkmcnt 15) folds its oldest positions.
    At joins the lists are aligned at the youngest end and unioned position by position, iterated to a fixed point (loop back
    edges: the attention Q prefetch is deliberately still pending at the back edge);
  * finding: an instruction that names a register overlapping a pending op's destination.  The one exception is a later op on the
    same in-order counter writing that register (VM after VM, LDS after LDS): a harmless write-after-write.  VGPR, AGPR and SGPR
    files are separate.

Not modelled, on purpose: write-after-read of store data (per LLVM only pre-CI hardware needs a wait there), MFMA / VALU wait states
(the asm MFMA `s_nop` padding of gemm_rowln.hip), ordering of LDS-DMA against `ds_read` through barriers (that needs address
reasoning), and memory-model fences.

    python -m tests.asm_hazards          per library: kernels, instructions analysed, VM / LGKM ops, findings
"""
from __future__ import annotations

import collections
import os
import re
import struct
import subprocess
import sys
import tempfile
from dataclasses import dataclass, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from vtamiq_amd import build  # noqa: E402

TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
VM_CAP, LGKM_CAP = 63, 15                    # s_waitcnt field widths on gfx9: vmcnt 6 bits, lgkmcnt 4 bits
LIBRARIES = {"libvtamiq_hip.so": ("_obj", build.LIB), "libvtamiq_hip_fp8.so": ("_obj_fp8", build.LIB_FP8)}


class AsmHazardError(RuntimeError):
    """The input cannot be analysed exactly (missing tool, unclassified memory op, indirect control flow, malformed text)."""


# ---- tools ---------------------------------------------------------------------------------------------------------------

def tool(name: str) -> str:
    """`name` from ROCm's llvm/bin: next to the hipcc that build.py uses, else under ROCM_PATH."""
    hipcc = os.path.realpath(build._hipcc())
    dirs = [os.path.join(os.path.dirname(hipcc), "..", "llvm", "bin"), os.path.dirname(hipcc)]
    if os.environ.get("ROCM_PATH"):
        dirs.append(os.path.join(os.environ["ROCM_PATH"], "llvm", "bin"))
    for d in dirs:
        p = os.path.join(d, name)
        if os.access(p, os.X_OK):
            return os.path.normpath(p)
    raise AsmHazardError(f"{name} not found in {dirs}")


def _run(cmd) -> str:
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def elf_section(path: str, name: str):
    """Bytes of section `name` of an ELF64 little-endian file, or None if it has no such section."""
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"\x7fELF" or data[4] != 2 or data[5] != 1:
        raise AsmHazardError(f"{path}: not an ELF64 little-endian object")
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)

    def header(i):                                       # (sh_name, sh_offset, sh_size)
        nm, _, _, _, off, size = struct.unpack_from("<IIQQQQ", data, shoff + i * shentsize)
        return nm, off, size

    _, stroff, _ = header(shstrndx)
    for i in range(shnum):
        nm, off, size = header(i)
        end = data.index(b"\0", stroff + nm)
        if data[stroff + nm:end].decode() == name:
            return data[off:off + size]
    return None


def disassemble_object(obj: str, workdir: str):
    """host object -> (disassembly, {mangled kernel: demangled}) of its gfx950 code object; None for a host-only object."""
    fatbin = elf_section(obj, ".hip_fatbin")
    if fatbin is None:
        return None
    stem = os.path.join(workdir, os.path.basename(obj))
    with open(stem + ".fatbin", "wb") as f:
        f.write(fatbin)
    _run([tool("clang-offload-bundler"), "--unbundle", "--type=o", f"--input={stem}.fatbin", f"--targets={TARGET}",
          f"--output={stem}.co"])
    return disassemble_code_object(stem + ".co")


_SYM = re.compile(r"^([0-9a-f]+)\s.*\s(F|O)\s+(\.\w+)\s+[0-9a-f]+\s+(?:\.(?:protected|hidden)\s+)?(.+)$")


def disassemble_code_object(co: str):
    """gfx950 code object -> (llvm-objdump disassembly, {mangled kernel: demangled}); the kernels are the symbols with a .kd
    descriptor, each of which must have a function symbol."""
    objdump = tool("llvm-objdump")
    text = _run([objdump, "-d", "--symbolize-operands", co])
    funcs, kds = {}, []
    for m in map(_SYM.match, _run([objdump, "-t", co]).splitlines()):
        if m and m.group(2) == "F":
            funcs[m.group(4)] = int(m.group(1), 16)
        elif m and m.group(4).endswith(".kd"):
            kds.append(m.group(4)[:-3])
    demangled = {int(m.group(1), 16): m.group(4)
                 for m in map(_SYM.match, _run([objdump, "-t", "-C", co]).splitlines()) if m and m.group(2) == "F"}
    missing = [k for k in kds if k not in funcs]
    if missing:
        raise AsmHazardError(f"{co}: kernel descriptors without a function symbol: {missing}")
    return text, {k: demangled.get(funcs[k], k) for k in kds}


# ---- instruction tables ---------------------------------------------------------------------------------------------------

VM, LDS, SMEM = "vmcnt", "lgkmcnt(LDS)", "lgkmcnt(SMEM)"

_VM_CLASSES = [                                      # (pattern, has a destination (first operand))
    (re.compile(r"(global|buffer|scratch)_load_lds_(dword(x[34])?|ubyte|sbyte|ushort|sshort)$"), False),
    (re.compile(r"(global|buffer|scratch)_load_(dword(x[234])?|ubyte|sbyte|ushort|sshort|short_d16(_hi)?|ubyte_d16(_hi)?"
                r"|sbyte_d16(_hi)?|format_\w+)$"), True),
    (re.compile(r"(global|buffer|scratch)_store_(dword(x[234])?|byte(_d16_hi)?|short(_d16_hi)?|format_\w+)$"), False),
    (re.compile(r"(global|buffer)_atomic_\w+$"), None),          # a destination only in the returning (sc0) form
    (re.compile(r"buffer_(wbl2|inv)$"), False),
]
_LDS_CLASSES = [
    (re.compile(r"ds_read\w*$"), True),                          # ds_read_*, ds_read2*, ds_read_b64_tr_b16, ds_read_addtid_b32
    (re.compile(r"ds_(bpermute|permute|swizzle)_b32$"), True),
    (re.compile(r"ds_\w+_rtn_\w+$"), True),
    (re.compile(r"ds_(append|consume)$"), True),
    (re.compile(r"ds_write\w*$"), False),
    (re.compile(r"ds_(add|sub|rsub|inc|dec|min|max|and|or|xor|mskor|cmpst|cmpswap|wrxchg\w*|pk_add)_\w+$"), False),
    (re.compile(r"ds_nop$"), False),
]
_SMEM_READS = ("s_memtime", "s_memrealtime")
_INDIRECT = ("s_setpc_b64", "s_swappc_b64", "s_call_b64", "s_rfe_b64", "s_cbranch_g_fork", "s_cbranch_join")
_ENDS = ("s_endpgm", "s_endpgm_saved", "s_endpgm_ordered_ps_done")
_REG = re.compile(r"(?<![\w.])([vas])(?:(\d+)|\[(\d+):(\d+)\])(?!\w)")
_FILE = {"v": 0, "a": 1, "s": 2}
_FIELD = re.compile(r"(vmcnt|expcnt|lgkmcnt)\((\d+)\)")


def regs_of(text: str) -> frozenset:
    """Register operands of an operand string: 'v7', 'v[4:7]', 'a[0:3]', 's[8:11]' -> {(file << 10) | index}; modifiers ignored."""
    out = set()
    for f, one, lo, hi in _REG.findall(text):
        base = _FILE[f] << 10
        if one:
            out.add(base | int(one))
        else:
            out.update(base | i for i in range(int(lo), int(hi) + 1))
    return frozenset(out)


def reg_name(r: int) -> str:
    return "vas"[r >> 10] + str(r & 1023)


def classify(mnemonic: str, operands: str):
    """-> (counter or None, destination present).  Raises on a memory mnemonic the tables do not classify."""
    if mnemonic.startswith("flat_"):
        raise AsmHazardError(f"flat memory op {mnemonic!r}: not expected in these kernels (it would count on both counters)")
    if mnemonic.startswith(("global_", "buffer_", "scratch_")):
        for pat, dest in _VM_CLASSES:
            if pat.match(mnemonic):
                mods = operands.split()
                if dest and "lds" in mods:
                    break                                # the buffer "lds" modifier form: not classified
                if dest is None:
                    dest = "sc0" in mods or "glc" in mods
                return VM, dest
        raise AsmHazardError(f"unclassified VM op {mnemonic!r} {operands!r}")
    if mnemonic.startswith("ds_"):
        for pat, dest in _LDS_CLASSES:
            if pat.match(mnemonic):
                return LDS, dest
        raise AsmHazardError(f"unclassified LDS op {mnemonic!r}")
    if mnemonic.startswith(("s_load", "s_buffer_load")) or mnemonic in _SMEM_READS:
        return SMEM, True
    return None, False


# ---- parsing ----------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Op:
    """One memory op in flight: where it was issued and which registers it will write."""
    addr: int
    text: str
    counter: str
    dest: frozenset


@dataclass
class Insn:
    addr: int
    mnemonic: str
    operands: str
    regs: frozenset                      # every register named
    counter: str = None
    dest: frozenset = frozenset()
    src: frozenset = frozenset()         # regs minus the destination operand (memory ops)
    op: Op = None

    @property
    def text(self):
        return f"{self.mnemonic} {self.operands}".strip()


@dataclass
class Finding:
    kernel: str
    insn_addr: int
    insn: str
    load_addr: int
    load: str
    counter: str
    regs: tuple
    wait: str

    def __str__(self):
        return (f"{self.kernel}\n    {self.insn_addr:#x}: {self.insn}  names {','.join(self.regs)}\n"
                f"    pending {self.counter} op {self.load_addr:#x}: {self.load}  -- needs s_waitcnt {self.wait} before it")


@dataclass
class KernelReport:
    name: str                            # mangled
    demangled: str
    instructions: int
    vm_ops: int
    lgkm_ops: int
    mnemonics: collections.Counter
    findings: list = field(default_factory=list)


_HEADER = re.compile(r"^([0-9a-fA-F]+) <([^>]+)>:\s*$")
_INSN = re.compile(r"^\s+([a-z_][\w.]*)(.*?)\s*//\s*([0-9a-fA-F]+):")
_LABEL = re.compile(r"L\d+$")


def split_functions(text: str):
    """llvm-objdump text -> {symbol: [(label or None, Insn) ...]}: `<Ln>` headers are labels inside the current symbol."""
    funcs, cur, label = {}, None, None
    for line in text.splitlines():
        m = _HEADER.match(line)
        if m:
            if _LABEL.match(m.group(2)):
                if cur is None:
                    raise AsmHazardError(f"label {m.group(2)} outside a symbol")
                label = m.group(2)
            else:
                cur = funcs.setdefault(m.group(2), [])
                label = None
            continue
        m = _INSN.match(line)
        if m:
            if cur is None:
                raise AsmHazardError(f"instruction outside a symbol: {line.strip()}")
            mn, ops = m.group(1), m.group(2).strip()
            ins = Insn(int(m.group(3), 16), mn, ops, regs_of(ops))
            counter, has_dest = classify(mn, ops)
            if counter:
                first = ops.split(",")[0] if has_dest else ""
                ins.counter, ins.dest = counter, regs_of(first)
                if has_dest and not ins.dest:
                    raise AsmHazardError(f"{ins.addr:#x}: {ins.text}: no destination register parsed")
                ins.src = regs_of(ops[len(first):])
                ins.op = Op(ins.addr, ins.text, counter, ins.dest)
            cur.append((label, ins))
            label = None
        elif line.strip() not in ("", "...") and not line.startswith("Disassembly of section") and "file format" not in line:
            raise AsmHazardError(f"unparsed line: {line!r}")
    return funcs


def build_cfg(name: str, body):
    """-> (blocks [[Insn]], edges [(taken target or None, fall-through or None)]) of one function; block 0 is the entry."""
    starts, label_at = {0}, {}
    for i, (label, ins) in enumerate(body):
        if label:
            starts.add(i)
            label_at[label] = i
        mn = ins.mnemonic
        if mn in _INDIRECT:
            raise AsmHazardError(f"{name}: indirect control flow at {ins.addr:#x}: {ins.text}")
        if mn.startswith(("s_cbranch", "s_branch")) or mn in _ENDS:
            starts.add(i + 1)
    starts = sorted(s for s in starts if s < len(body))
    index = {s: k for k, s in enumerate(starts)}
    blocks, edges = [], []
    for k, s in enumerate(starts):
        e = starts[k + 1] if k + 1 < len(starts) else len(body)
        insns = [ins for _, ins in body[s:e]]
        last = insns[-1]
        mn = last.mnemonic
        nxt = index[e] if e < len(body) else None
        blocks.append(insns)
        if mn.startswith(("s_cbranch", "s_branch")):
            tgt = last.operands.strip()
            if not _LABEL.match(tgt) or tgt not in label_at:
                raise AsmHazardError(f"{name}: branch to a non-label target at {last.addr:#x}: {last.text}")
            edges.append((index[label_at[tgt]], nxt if mn.startswith("s_cbranch") else None))
        else:
            edges.append((None, None if mn in _ENDS else nxt))
    return blocks, edges


# ---- the abstract state -------------------------------------------------------------------------------------------------------
# Pending = (vm, lds, smem): vm / lds tuples of positions (frozensets of Op), oldest first; smem a frozenset of Op.
#
# One piece of path sensitivity, so that the compiler's lowering of `if (a) wait(x); else if (b) wait(y); else wait(z);` is not
# read as a path that skips every wait: hipcc threads such chains through a 64-bit SGPR flag set by `s_mov_b64 s[i:i+1], 0 / -1`
# and tested by `s_and(n2)_b64 vcc, exec, s[i:i+1]` + `s_cbranch_vccz / vccnz`.  The state is split by the flags known constant
# (a key), and a branch on a vcc that is known ZERO follows one edge.  Nothing assumes exec != 0: a vcc = exec test keeps both.

EMPTY = ((), (), frozenset())
NO_FLAGS = (frozenset(), False)                  # (frozenset of (lowest SGPR of a pair, 0 | -1)), vcc known zero)
MAX_KEYS = 16                                    # more flag combinations at one block: drop the flags (sound, less precise)
_SET_FLAG = re.compile(r"s\[(\d+):(\d+)\], (0|-1)$")
_TEST_FLAG = re.compile(r"vcc, exec, s\[(\d+):(\d+)\]$")
_SGPR = _FILE["s"] << 10


def _fold(lst, cap):
    if len(lst) <= cap:
        return lst
    k = len(lst) - cap + 1
    return (frozenset().union(*lst[:k]),) + lst[k:]


def _keep(lst, n):
    return lst[len(lst) - n:] if n < len(lst) else lst


def _merge_lists(a, b):
    if len(a) < len(b):
        a, b = b, a
    d = len(a) - len(b)
    return a[:d] + tuple(x | y for x, y in zip(a[d:], b))


def merge(s, t):
    """Join of two pending states: lists aligned at the youngest end, unioned position by position."""
    return (_merge_lists(s[0], t[0]), _merge_lists(s[1], t[1]), s[2] | t[2])


def _flags_step(ins, flags):
    consts, vcc_zero = flags
    mn, ops = ins.mnemonic, ins.operands
    m = _TEST_FLAG.match(ops) if mn in ("s_and_b64", "s_andn2_b64") else None
    if m:
        v = dict(consts).get(int(m.group(1)))
        return consts, (v == 0) if mn == "s_and_b64" else (v == -1)
    if "vcc" in ops:
        vcc_zero = False
    sg = {r & 1023 for r in ins.regs if r >> 10 == 2}
    if sg and consts:
        consts = frozenset((lo, v) for lo, v in consts if lo not in sg and lo + 1 not in sg)
    m = _SET_FLAG.match(ops) if mn == "s_mov_b64" else None
    if m and int(m.group(2)) == int(m.group(1)) + 1:
        consts = consts | {(int(m.group(1)), int(m.group(3)))}
    return consts, vcc_zero


def _wait_for(lst, i, counter):
    """The wait that retires position i of `lst`: every younger position may stay in flight."""
    younger = len(lst) - 1 - i
    return f"vmcnt({younger})" if counter == VM else f"lgkmcnt({younger})"


def transfer(state, flags, insns, kernel=None, findings=None):
    vm, lds, smem = state
    pend = None                                              # union of every pending destination (cached)
    for ins in insns:
        if findings is not None and ins.regs:
            if pend is None:
                pend = frozenset().union(*(op.dest for pos in vm + lds for op in pos), *(op.dest for op in smem))
            if not pend.isdisjoint(ins.regs):
                _check(ins, vm, lds, smem, kernel, findings)
        flags = _flags_step(ins, flags)                      # every instruction: VALU writes (v_cmp_* s[..] / vcc, v_readlane) too
        mn = ins.mnemonic
        if mn == "s_waitcnt":
            fields = dict(_FIELD.findall(ins.operands))
            if _FIELD.sub("", ins.operands).strip():
                raise AsmHazardError(f"{ins.addr:#x}: unparsed s_waitcnt operands {ins.operands!r}")
            if "vmcnt" in fields:
                vm = _keep(vm, int(fields["vmcnt"]))
            if "lgkmcnt" in fields:
                n = int(fields["lgkmcnt"])
                lds = _keep(lds, n)
                if n == 0:
                    smem = frozenset()
            pend = None
        elif mn.startswith("s_waitcnt"):
            raise AsmHazardError(f"{ins.addr:#x}: unmodelled wait {ins.text}")
        elif ins.counter == VM:
            vm = _fold(vm + (frozenset((ins.op,)),), VM_CAP)
            pend = None
        elif ins.counter == LDS:
            lds = _fold(lds + (frozenset((ins.op,)),), LGKM_CAP)
            pend = None
        elif ins.counter == SMEM:
            smem = smem | {ins.op}
            pend = None
    return (vm, lds, smem), flags


def _check(ins, vm, lds, smem, kernel, findings):
    # a later op on the same in-order counter may write a pending destination (write-after-write in order); anything else that
    # names it -- a read, a VALU / SALU write, an op of the other counter -- is a hazard
    def add(op, h, counter, wait):
        findings.append(Finding(kernel, ins.addr, ins.text, op.addr, op.text, counter, tuple(reg_name(r) for r in sorted(h)), wait))

    for counter, lst in ((VM, vm), (LDS, lds)):
        regs = ins.src if ins.counter == counter else ins.regs
        seen = set()
        for i in range(len(lst) - 1, -1, -1):              # youngest first: an op merged into several positions needs the smallest wait
            for op in lst[i]:
                h = op.dest & regs
                if h and op not in seen:
                    seen.add(op)
                    add(op, h, counter, _wait_for(lst, i, counter))
    for op in smem:
        h = op.dest & ins.regs
        if h:
            add(op, h, SMEM, "lgkmcnt(0)")


def _successors(edges, insns, flags):
    taken, fall = edges
    last = insns[-1].mnemonic
    if flags[1] and last == "s_cbranch_vccz":
        return [taken]
    if flags[1] and last == "s_cbranch_vccnz":
        return [fall] if fall is not None else []
    return [s for s in (taken, fall) if s is not None]


def _join(states, flags, new):
    """Add `new` under key `flags` to a block's {flags: pending}; -> the updated dict, or None if nothing changed."""
    old = states.get(flags)
    val = new if old is None else merge(old, new)
    if val == old:
        return None
    out = dict(states)
    out[flags] = val
    if len(out) > MAX_KEYS:
        acc = EMPTY
        for v in out.values():
            acc = merge(acc, v)
        out = {NO_FLAGS: acc}
        if out == states:
            return None
    return out


def analyze_function(name: str, body, demangled: str = None) -> KernelReport:
    demangled = demangled or name
    blocks, edges = build_cfg(name, body)
    state_in = {0: {NO_FLAGS: EMPTY}}
    work, queued = [0], {0}
    while work:
        b = work.pop()
        queued.discard(b)
        for flags, st in list(state_in[b].items()):
            out, oflags = transfer(st, flags, blocks[b])
            for s in _successors(edges[b], blocks[b], oflags):
                upd = _join(state_in.get(s, {}), oflags, out)
                if upd is not None:
                    state_in[s] = upd
                    if s not in queued:
                        queued.add(s)
                        work.append(s)
    findings, seen = [], set()
    for b in sorted(state_in):
        raw = []
        for flags, st in state_in[b].items():
            transfer(st, flags, blocks[b], demangled, raw)
        for f in raw:
            if (f.insn_addr, f.load_addr) not in seen:
                seen.add((f.insn_addr, f.load_addr))
                findings.append(f)
    reached = [ins for b in state_in for ins in blocks[b]]
    mnem = collections.Counter(ins.mnemonic for ins in reached if ins.counter)
    return KernelReport(name, demangled, len(reached), sum(1 for i in reached if i.counter == VM),
                        sum(1 for i in reached if i.counter in (LDS, SMEM)), mnem,
                        sorted(findings, key=lambda f: (f.insn_addr, f.load_addr)))


def analyze_text(text: str, demangled=None):
    """Disassembly text -> {symbol: KernelReport} for every function in it."""
    demangled = demangled or {}
    return {n: analyze_function(n, body, demangled.get(n)) for n, body in split_functions(text).items()}


# ---- the shipped objects --------------------------------------------------------------------------------------------------------

@dataclass
class ObjectReport:
    source: str
    path: str
    device: bool                         # False: a host-only object (no .hip_fatbin section)
    kernel_symbols: dict                 # mangled -> demangled, from the kernel descriptors (.kd)
    kernels: dict                        # mangled -> KernelReport, from the disassembly


def analyze_object(obj: str, workdir: str = None) -> ObjectReport:
    with tempfile.TemporaryDirectory(dir=workdir) as tmp:
        dis = disassemble_object(obj, tmp)
    src = os.path.basename(obj).replace(".o", ".hip")
    if dis is None:
        return ObjectReport(src, obj, False, {}, {})
    text, kernels = dis
    return ObjectReport(src, obj, True, kernels, analyze_text(text, kernels))


def shipped_objects(objdir: str, lib: str):
    """The objects build.py links into `lib`: exactly one per build.SOURCES entry, none older than the library."""
    d = os.path.join(build.CSRC, objdir)
    have = sorted(f for f in os.listdir(d) if f.endswith(".o"))
    want = sorted(s.replace(".hip", ".o") for s in build.SOURCES)
    if have != want:
        raise AsmHazardError(f"{d}: objects {have} != build.SOURCES {want}")
    if not os.path.exists(lib):
        raise AsmHazardError(f"{lib} is not built")
    objs = [os.path.join(d, f) for f in want]
    for o in objs:
        if os.path.getmtime(o) > os.path.getmtime(lib):
            raise AsmHazardError(f"{o} is newer than {lib}: the library does not hold it")
    return objs


def main() -> int:
    total = 0
    for libname, (objdir, lib) in LIBRARIES.items():
        reports = [analyze_object(o) for o in shipped_objects(objdir, lib)]
        ks = [k for r in reports for k in r.kernels.values()]
        n_find = sum(len(k.findings) for k in ks)
        total += n_find
        print(f"{libname}: {len(reports)} objects, {len(ks)} kernels, {sum(k.instructions for k in ks)} instructions analysed, "
              f"{sum(k.vm_ops for k in ks)} VM ops, {sum(k.lgkm_ops for k in ks)} LGKM ops, {n_find} findings")
        for r in reports:
            rk = list(r.kernels.values())
            print(f"  {r.source:22s} " + (f"{len(rk):3d} kernels {sum(k.instructions for k in rk):7d} insns "
                                          f"{sum(k.vm_ops for k in rk):6d} VM {sum(k.lgkm_ops for k in rk):6d} LGKM "
                                          f"{sum(len(k.findings) for k in rk):3d} findings" if r.device else "host code only"))
            for k in rk:
                for f in k.findings:
                    print("    " + str(f).replace("\n", "\n    "))
    return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main())
