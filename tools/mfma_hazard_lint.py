#!/usr/bin/env python3
"""MFMA hazard check of the hand-issued (inline asm) MFMAs in the device assembly.

hipcc pads the hazards of the instructions it generates, but not of instructions inside asm strings: an MFMA issued
from inline asm relies on hand-placed pads (sq_dense_scan.hpp mfma_fence_in / mfma_fence_out, sq_itq_wide.hpp).  This
tool compiles every unit whose sources hold an inline `v_mfma` to gfx950 assembly with the Makefile's flags and walks
every control-flow path out of (R1) and into (R2) each inline MFMA:

  R1  the D registers of an inline MFMA are read or written by a non-MFMA instruction, or read as A / B by another
      MFMA, fewer than 12 wait states after it;
  R2  a VALU, LDS or VMEM write of a register is followed, fewer than 2 wait states later, by an inline MFMA that
      reads it as A, B or C.

Wait states are counted the way hipcc's hazard recognizer counts them: one per instruction (an intervening MFMA is
one state, not its 32 cycles), N + 1 for `s_nop N`, none for labels and empty asm blocks.  tests/test_isa_hazards.py
checks that hipcc's own padding of the builtin MFMA still matches these numbers.  Overwriting an MFMA's A / B source
registers right after it is not a hazard (hipcc pads nothing there) and is not checked.

    python tools/mfma_hazard_lint.py                 # compile and check; exit 1 when there are findings
    python tools/mfma_hazard_lint.py --asm X.s ...   # check existing assembly files
    python tools/mfma_hazard_lint.py --keep DIR      # keep the generated .s files in DIR
"""
import argparse
import os
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "smqtk_indexing_amd", "csrc")

D_STATES = 12  # R1: MFMA result -> any other reader / writer (gfx950, 8- and 16-pass XDL ops: what hipcc pads)
SRC_STATES = 2  # R2: VALU / memory write of A, B or C -> MFMA read

_MFMA_STR = re.compile(r'"[^"\n]*v_mfma')  # v_mfma inside a string literal: an asm statement, not a comment
_INCLUDE = re.compile(r'^\s*#\s*include\s*"([^"]+)"', re.M)
_REG = re.compile(r"\b([va])(?:\[(\d+):(\d+)\]|(\d+)(?!\w))")
_LABEL = re.compile(r"^([.\w$]+):")
_TYPE_FN = re.compile(r"^\s*\.type\s+([.\w$]+),\s*@function")
_NOP = re.compile(r"^s_nop\s+(0x[0-9a-fA-F]+|\d+)")


# ------------------------------------------------------------------ inputs

def _sources_with_inline_mfma(path, seen):
    """True when `path` or a local header it includes holds an asm string with v_mfma."""
    if path in seen:
        return False
    seen.add(path)
    try:
        text = open(path).read()
    except OSError:
        return False
    if _MFMA_STR.search(text):
        return True
    for inc in _INCLUDE.findall(text):
        if _sources_with_inline_mfma(os.path.join(os.path.dirname(path), inc), seen):
            return True
    return False


def units_with_inline_mfma(csrc=CSRC):
    """The Makefile's SRCS whose translation unit holds an inline MFMA."""
    return [u for u in makefile_sources(csrc) if _sources_with_inline_mfma(os.path.join(csrc, u), set())]


def _makefile_vars(csrc):
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    out = {}
    for m in re.finditer(r"^(\w+)\s*[?:]?=\s*(.*)$", text, re.M):
        out.setdefault(m.group(1), m.group(2).strip())
    return out


def makefile_sources(csrc=CSRC):
    return _makefile_vars(csrc)["SRCS"].split()


def makefile_flags(csrc=CSRC, arch="gfx950"):
    v = _makefile_vars(csrc)
    return [f.replace("$(ARCH)", arch) for f in shlex.split(v["CXXFLAGS"])]


def hipcc_path():
    p = os.environ.get("HIPCC") or "/opt/rocm/bin/hipcc"
    return p if os.path.isfile(p) and os.access(p, os.X_OK) else None


def compile_to_asm(src, out_s, flags=None, csrc=CSRC):
    """hipcc --cuda-device-only -S of one unit with the Makefile's flags (or `flags`)."""
    hipcc = hipcc_path()
    if hipcc is None:
        raise RuntimeError("hipcc not found (set HIPCC)")
    cmd = [hipcc] + (makefile_flags(csrc) if flags is None else list(flags)) + ["--cuda-device-only", "-S", src, "-o", out_s]
    r = subprocess.run(cmd, cwd=os.path.dirname(os.path.abspath(src)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       universal_newlines=True)
    if r.returncode != 0:
        raise RuntimeError("hipcc failed on %s:\n%s" % (src, r.stdout[-4000:]))
    return out_s


def compile_units(units, outdir, jobs=4, csrc=CSRC):
    """{unit: path of its .s} for the units (at most `jobs` hipcc processes at a time)."""
    jobs = max(1, min(4, jobs))
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        futs = {u: ex.submit(compile_to_asm, os.path.join(csrc, u), os.path.join(outdir, os.path.splitext(u)[0] + ".s"))
                for u in units}
        return {u: f.result() for u, f in futs.items()}


# ------------------------------------------------------------------ parsing

def _regs(text):
    """v / a registers named in an operand string, as a set of ('v' | 'a', index)."""
    out = set()
    for cls, lo, hi, one in _REG.findall(text):
        if one:
            out.add((cls, int(one)))
        else:
            out.update((cls, i) for i in range(int(lo), int(hi) + 1))
    return out


def _split_operands(rest):
    ops, depth, cur = [], 0, ""
    for ch in rest:
        if ch == "[":
            depth += 1
        elif ch == "]":
            depth -= 1
        if ch == "," and depth == 0:
            ops.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        ops.append(cur.strip())
    return ops


@dataclass
class Inst:
    line: int  # 1-based line in the .s
    mnem: str
    ops: list
    inline: bool  # between ;;#ASMSTART and ;;#ASMEND
    states: int
    mfma: bool
    regs: set = field(default_factory=set)  # every v / a register named
    defs: set = field(default_factory=set)  # v / a registers written (VALU / LDS / VMEM results; MFMA D)
    src: set = field(default_factory=set)  # MFMA: registers read as A / B
    srcc: set = field(default_factory=set)  # MFMA: registers read as C
    target: str = None  # branch target label
    cond: bool = False  # conditional branch
    end: bool = False  # no fall-through (end of program, return, unconditional branch)


_VMEM = ("global_", "buffer_", "flat_", "scratch_")


def _classify(mnem, ops, inst):
    if mnem.startswith("v_mfma") or mnem.startswith("v_smfmac"):
        inst.mfma = True
        if ops:
            inst.defs = _regs(ops[0])
        inst.src = set().union(*[_regs(o) for o in ops[1:3]]) if len(ops) > 2 else set()
        inst.srcc = _regs(ops[3]) if len(ops) > 3 else set()
        return
    # results in v / a registers: the first operand of a vector ALU op; of an LDS / VMEM op that returns data (loads,
    # returning atomics, permutes) -- memory ops that only write memory, and loads straight into LDS, have none
    if mnem.startswith("v_") and ops:
        inst.defs = _regs(ops[0])
    elif mnem.startswith("ds_") and ops:
        if not any(w in mnem for w in ("write", "store", "_nop", "gws", "append", "consume")) and (
                "read" in mnem or "load" in mnem or "rtn" in mnem or "permute" in mnem or "swizzle" in mnem):
            inst.defs = _regs(ops[0])
    elif mnem.startswith(_VMEM) and ops:
        returns = ("load" in mnem and "_lds" not in mnem) or ("atomic" in mnem and "glc" in " ".join(ops[1:]))
        if returns:
            inst.defs = _regs(ops[0])


def _nop_states(mnem_line):
    m = _NOP.match(mnem_line)
    return int(m.group(1), 0) + 1 if m else None


@dataclass
class Function:
    name: str
    insts: list  # Inst
    labels: dict  # label -> index of the first instruction after it
    succ: list = None  # per block start index ... (built by cfg())


def parse_asm(text):
    """[Function] of an assembly file (instructions with their .s line numbers, labels)."""
    fn_names = set(m.group(1) for m in map(_TYPE_FN.match, text.splitlines()) if m)
    funcs, cur = [], None
    inline = False
    for ln, raw in enumerate(text.splitlines(), 1):
        s = raw.strip()
        if s.startswith(";;#ASMSTART"):
            inline = True
            continue
        if s.startswith(";;#ASMEND"):
            inline = False
            continue
        code = s.split(";", 1)[0].split("//", 1)[0].strip()
        if not code:
            continue
        m = _LABEL.match(code)
        if m:
            name = m.group(1)
            if name in fn_names:
                cur = Function(name, [], {})
                funcs.append(cur)
            elif name.startswith(".Lfunc_end"):
                cur = None
            elif cur is not None:
                cur.labels[name] = len(cur.insts)
            code = code[m.end():].strip()
            if not code:
                continue
        if cur is None or code.startswith("."):
            continue
        for piece in code.split("\n"):
            parts = piece.split(None, 1)
            mnem = parts[0]
            rest = parts[1] if len(parts) > 1 else ""
            ops = _split_operands(rest)
            nop = _nop_states(piece)
            inst = Inst(ln, mnem, ops, inline, nop if nop is not None else 1, False)
            if not mnem.startswith("s_"):
                inst.regs = _regs(rest)
                _classify(mnem, ops, inst)
            elif mnem == "s_branch":
                inst.target, inst.end = ops[0] if ops else None, True
            elif mnem.startswith("s_cbranch_"):
                inst.target, inst.cond = ops[0] if ops else None, True
            elif mnem in ("s_endpgm", "s_setpc_b64", "s_endpgm_saved", "s_trap"):
                inst.end = True
            cur.insts.append(inst)
    return funcs


def _succ(fn, i):
    """Indices an execution can continue at after instruction i, each with whether it is a taken branch."""
    ins = fn.insts[i]
    out = []
    if ins.target is not None and ins.target in fn.labels:
        out.append((fn.labels[ins.target], True))
    if not ins.end and i + 1 < len(fn.insts):
        out.append((i + 1, False))
    return out


def _pred_map(fn):
    pred = {}
    for i in range(len(fn.insts)):
        for j, taken in _succ(fn, i):
            pred.setdefault(j, []).append((i, taken))
    return pred


# ------------------------------------------------------------------ rules

@dataclass
class Finding:
    rule: str
    function: str
    producer_line: int
    reader_line: int
    states: int  # wait states between the two instructions (exclusive)
    mfmas_between: int
    branch_taken: bool
    producer: str
    reader: str

    def format(self):
        return ("%s %s\n    producer .s:%d  %s\n    reader   .s:%d  %s\n    %d wait states (need %d), %d MFMA(s) between, %s"
                % (self.rule, self.function, self.producer_line, self.producer, self.reader_line, self.reader, self.states,
                   D_STATES if self.rule == "R1" else SRC_STATES, self.mfmas_between,
                   "through a taken branch" if self.branch_taken else "fall-through only"))


def _text(ins):
    return (ins.mnem + " " + ", ".join(ins.ops)).strip()


def _r1_hits(ins, live):
    if ins.mfma:
        return bool(ins.src & live)
    return bool(ins.regs & live)


def walk_forward(fn, i0, regs, need, hit, kill=None):
    """Shortest paths from instruction i0 to instructions j that `hit(insts[j], live)`, fewer than `need` states
    after it; `kill(ins)` gives registers an instruction takes out of the live set.  {j: (states, mfmas, taken)}."""
    best = {}
    seen = {}
    stack = [(i0, 0, 0, False, frozenset(regs))]
    while stack:
        i, st, nm, taken, live = stack.pop()
        for j, tk in _succ(fn, i):
            key = (j, live)
            t = taken or tk
            if key in seen and seen[key] <= (st, not t):
                continue
            seen[key] = (st, not t)
            ins = fn.insts[j]
            if hit(ins, live):
                if j not in best or (st, not t) < (best[j][0], not best[j][2]):
                    best[j] = (st, nm, t)
                continue  # the first reader on a path is the one that matters
            nst = st + ins.states
            if nst >= need:
                continue
            nlive = live - kill(ins) if kill else live
            if not nlive:
                continue
            stack.append((j, nst, nm + (1 if ins.mfma else 0), t, frozenset(nlive)))
    return best


def walk_backward(fn, pred, i0, regs, need):
    """Shortest paths back from the MFMA at i0 to a VALU / LDS / VMEM write of one of `regs` fewer than `need`
    states before it.  {j: (states, mfmas, taken)}."""
    best = {}
    seen = {}
    stack = [(i0, 0, 0, False)]
    while stack:
        i, st, nm, taken = stack.pop()
        for j, tk in pred.get(i, ()):
            t = taken or tk
            if j in seen and seen[j] <= (st, not t):
                continue
            seen[j] = (st, not t)
            ins = fn.insts[j]
            if not ins.mfma and ins.defs & regs:
                if j not in best or (st, not t) < (best[j][0], not best[j][2]):
                    best[j] = (st, nm, t)
                continue
            nst = st + ins.states
            if nst >= need:
                continue
            stack.append((j, nst, nm + (1 if ins.mfma else 0), t))
    return best


def check_function(fn, inline_only=True):
    """Findings of R1 and R2 for the inline MFMAs of one function (all MFMAs when not inline_only)."""
    out = []
    pred = None
    for i, ins in enumerate(fn.insts):
        if not ins.mfma or (inline_only and not ins.inline):
            continue
        d = ins.defs
        hits = walk_forward(fn, i, d, D_STATES, _r1_hits, kill=lambda x: x.defs if x.mfma else set())
        for j, (st, nm, tk) in sorted(hits.items()):
            out.append(Finding("R1", fn.name, ins.line, fn.insts[j].line, st, nm, tk, _text(ins), _text(fn.insts[j])))
        if pred is None:
            pred = _pred_map(fn)
        back = walk_backward(fn, pred, i, ins.src | ins.srcc, SRC_STATES)
        for j, (st, nm, tk) in sorted(back.items()):
            out.append(Finding("R2", fn.name, fn.insts[j].line, ins.line, st, nm, tk, _text(fn.insts[j]), _text(ins)))
    return out


def check_asm(text, functions=None):
    """Findings in an assembly text (optionally only the functions whose name is in `functions`)."""
    out = []
    for fn in parse_asm(text):
        if functions is None or fn.name in functions:
            out.extend(check_function(fn))
    return out


def min_states(fn, i, rule_hit=None):
    """Shortest distance (states, mfmas, taken, reader index) from MFMA i to the first non-MFMA reader / writer of
    its D registers or MFMA A / B reader -- for calibrating against hipcc's own pads (any MFMA, not only inline)."""
    hits = walk_forward(fn, i, fn.insts[i].defs, 1 << 30, rule_hit or _r1_hits,
                        kill=lambda x: x.defs if x.mfma else set())
    if not hits:
        return None
    j = min(hits, key=lambda k: hits[k][0])
    return hits[j] + (j,)


# ------------------------------------------------------------------ demangling of the scan kernels' names

_MANGLED = re.compile(r"^_ZN2sq(L?)(\d+)(\w+)$")


def template_name(sym):
    """`dense_scan_kernel<4,4,1,4,1,true,false,true>` for a mangled sq:: function template instance with integer /
    bool arguments; None otherwise."""
    m = _MANGLED.match(sym)
    if not m:
        return None
    n = int(m.group(2))
    rest = m.group(3)
    name, rest = rest[:n], rest[n:]
    if not rest.startswith("I"):
        return None
    args = []
    rest = rest[1:]
    while rest.startswith("L"):
        a = re.match(r"L([ib])(n?\d+)E", rest)
        if not a:
            return None
        v = a.group(2).replace("n", "-")
        args.append(("true" if v == "1" else "false") if a.group(1) == "b" else v)
        rest = rest[a.end():]
    if not rest.startswith("E"):
        return None
    return "%s<%s>" % (name, ",".join(args))


def function_names(text):
    return [m.group(1) for m in map(_TYPE_FN.match, text.splitlines()) if m]


# ------------------------------------------------------------------ driver

def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--asm", nargs="*", help="check these .s files instead of compiling")
    ap.add_argument("--keep", help="write the .s files here (default: a temporary directory)")
    ap.add_argument("-j", "--jobs", type=int, default=4, help="parallel hipcc jobs (at most 4)")
    args = ap.parse_args(argv)
    if args.asm:
        files = {os.path.basename(p): p for p in args.asm}
        tmp = None
    else:
        units = units_with_inline_mfma()
        print("units with inline MFMAs: %s" % " ".join(units), flush=True)
        tmp = None if args.keep else tempfile.TemporaryDirectory()
        outdir = args.keep or tmp.name
        os.makedirs(outdir, exist_ok=True)
        files = compile_units(units, outdir, args.jobs)
    total = 0
    try:
        for unit, path in sorted(files.items()):
            text = open(path).read()
            found = check_asm(text)
            n_inline = sum(1 for fn in parse_asm(text) for x in fn.insts if x.mfma and x.inline)
            print("%s: %d inline MFMAs, %d findings" % (unit, n_inline, len(found)))
            for f in found:
                name = template_name(f.function) or f.function
                print("  [%s] %s" % (name, f.format()))
            total += len(found)
    finally:
        if tmp is not None:
            tmp.cleanup()
    print("%d finding(s)" % total)
    return 1 if total else 0


if __name__ == "__main__":
    sys.exit(main())
