"""
MFMA hazards of the hand-issued (inline asm) MFMAs, checked in the gfx950 assembly on the CPU
(tools/mfma_hazard_lint.py): hipcc pads the hazards of what it generates, not of what sits inside asm strings.

* calibration: hipcc's own pads around the builtin MFMA still match the lint's wait-state counting;
* negative controls: small inline-asm kernels the lint must flag (or pass);
* the shipped units: no finding;
* census: every scan-kernel instantiation in the assembly has a forcing recipe in
  tests/test_hip_scan_variants.py (SCAN_VARIANTS), so a new build cannot go untested on the GPU.
"""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("mfma_hazard_lint", os.path.join(ROOT, "tools", "mfma_hazard_lint.py"))
L = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(L)

pytestmark = pytest.mark.skipif(L.hipcc_path() is None, reason="hipcc is not installed: nothing to compile the assembly with")

_CLOBBER = ", ".join('"v%d"' % i for i in range(25))
_MFMA = "v_mfma_f32_32x32x16_bf16 v[0:15], v[16:19], v[20:23], v[0:15]"

# Builtin MFMAs (hipcc pads them: calibration) and inline-asm controls with fixed registers (nobody pads them).
PROBE_SRC = r"""
#include <hip/hip_runtime.h>
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// the result read by a VALU right after the MFMA
extern "C" __global__ void cal_read(const bf16x8* a, const bf16x8* b, float* out) {
    const int l = threadIdx.x;
    f32x16 acc = {};
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[l], b[l], acc, 0, 0, 0);
    out[l] = acc[0] * acc[1];
}
// the same read with four independent MFMAs in between
extern "C" __global__ void cal_between(const bf16x8* a, const bf16x8* b, float* out) {
    const int l = threadIdx.x;
    const f32x16 z = {};
    const f32x16 p = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[l], b[l], z, 0, 0, 0);
    const f32x16 q0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[l + 64], b[l], z, 0, 0, 0);
    const f32x16 q1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[l + 128], b[l], z, 0, 0, 0);
    const f32x16 q2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[l + 192], b[l], z, 0, 0, 0);
    const f32x16 q3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[l + 256], b[l], z, 0, 0, 0);
    float s = p[0] * p[1];
    s += q0[0] * q0[1];
    s += q1[0] * q1[1];
    s += q2[0] * q2[1];
    s += q3[0] * q3[1];
    out[l] = s;
}
// the A operand overwritten by the next load right after the MFMA that read it
extern "C" __global__ void cal_war(const bf16x8* a, const bf16x8* b, float* out, int n) {
    const int l = threadIdx.x;
    f32x16 acc = {};
    const bf16x8 bb = b[l];
    bf16x8 x = a[l];
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x, bb, acc, 0, 0, 0);
        x = a[l + 64 * (i + 1)];
    }
    out[l] = acc[0];
}

extern "C" __global__ void hz_unpadded() {
    asm volatile("MFMA\n\tv_add_f32 v24, v0, v1" ::: CLOBBER);
}
extern "C" __global__ void hz_padded() {
    asm volatile("MFMA\n\ts_nop 11\n\tv_add_f32 v24, v0, v1" ::: CLOBBER);
}
// padded on the fall-through path only: the branch reaches the read one state after the MFMA
extern "C" __global__ void hz_branch(int flag) {
    asm volatile("s_cmp_eq_u32 %0, 0\n\t"
                 "MFMA\n\t"
                 "s_cbranch_scc1 .Lhz_branch_read\n\t"
                 "s_nop 11\n"
                 ".Lhz_branch_read:\n\t"
                 "v_add_f32 v24, v0, v1" ::"s"(flag) : CLOBBER, "scc");
}
// a VALU writes the A operand right before the MFMA
extern "C" __global__ void hz_src() {
    asm volatile("v_mov_b32 v16, 0\n\tMFMA" ::: CLOBBER);
}
""".replace("MFMA", _MFMA).replace("CLOBBER", _CLOBBER)


@pytest.fixture(scope="module")
def probe_asm(tmp_path_factory):
    d = tmp_path_factory.mktemp("isa_probe")
    src = d / "probe.hip"
    src.write_text(PROBE_SRC)
    s = L.compile_to_asm(str(src), str(d / "probe.s"))
    return {fn.name: fn for fn in L.parse_asm(open(s).read())}


@pytest.fixture(scope="module")
def shipped_asm(tmp_path_factory):
    """The shipped units with inline MFMAs compiled once (Makefile flags) for every test of the module."""
    d = tmp_path_factory.mktemp("isa_units")
    units = L.units_with_inline_mfma()
    files = L.compile_units(units, str(d), jobs=4)
    return {u: open(p).read() for u, p in files.items()}


def _mfmas(fn):
    return [i for i, x in enumerate(fn.insts) if x.mfma]


# ------------------------------------------------------------------ calibration

def test_calibration_result_read_needs_12_states(probe_asm):
    fn = probe_asm["cal_read"]
    (i,) = _mfmas(fn)
    states, mfmas, taken, j = L.min_states(fn, i)
    assert fn.insts[j].mnem.startswith("v_") and mfmas == 0
    # hipcc pads exactly what the lint demands: more would mean the lint's 12 is too short
    assert states == L.D_STATES, "hipcc pads %d states between the MFMA and a VALU read of its result" % states


def test_calibration_an_mfma_in_between_counts_one_state(probe_asm):
    fn = probe_asm["cal_between"]
    res = [L.min_states(fn, i) for i in _mfmas(fn)]
    assert len(res) == 5 and all(r is not None for r in res)
    # every result read at 12 states or more counted one per MFMA, and at least one read sits exactly at 12 with
    # MFMAs in between: hipcc then counts each of them as one state (were it more, its pad would be shorter)
    assert min(r[0] for r in res) >= L.D_STATES
    assert any(r[0] == L.D_STATES and r[1] >= 1 for r in res), res


def test_calibration_a_operand_overwrite_is_not_padded(probe_asm):
    fn = probe_asm["cal_war"]
    (i,) = _mfmas(fn)
    a_regs = L._regs(fn.insts[i].ops[1])
    hits = L.walk_forward(fn, i, a_regs, L.D_STATES, lambda x, live: not x.mfma and bool(x.defs & live))
    assert hits, "no overwrite of the A operand found after the MFMA"
    j = min(hits, key=lambda k: hits[k][0])
    # the next iteration's load lands in the registers the MFMA just read, behind the loop branch and one address
    # instruction: no pad (a rule there would need several states)
    assert fn.insts[j].mnem.startswith("global_load"), fn.insts[j]
    assert hits[j][0] <= 2, "hipcc pads %d states before an overwrite of an MFMA's A operand" % hits[j][0]


# ------------------------------------------------------------------ negative controls

def test_control_unpadded_read_is_flagged(probe_asm):
    f = L.check_function(probe_asm["hz_unpadded"])
    assert len(f) == 1 and f[0].rule == "R1" and f[0].states == 0 and not f[0].branch_taken, [x.format() for x in f]


def test_control_padded_read_is_clean(probe_asm):
    assert L.check_function(probe_asm["hz_padded"]) == []


def test_control_read_reached_through_a_branch_is_flagged(probe_asm):
    f = L.check_function(probe_asm["hz_branch"])
    assert len(f) == 1 and f[0].rule == "R1" and f[0].branch_taken and f[0].states == 1, [x.format() for x in f]


def test_control_source_written_right_before_the_mfma_is_flagged(probe_asm):
    f = L.check_function(probe_asm["hz_src"])
    assert len(f) == 1 and f[0].rule == "R2" and f[0].states == 0, [x.format() for x in f]


# ------------------------------------------------------------------ the shipped units

def test_units_with_inline_mfma_are_found():
    units = L.units_with_inline_mfma()
    assert "sq_dense.hip" in units and "sq_itq.hip" in units, units


def test_shipped_units_have_no_mfma_hazards(shipped_asm):
    report = []
    n_inline = 0
    for unit, text in sorted(shipped_asm.items()):
        for fn in L.parse_asm(text):
            n_inline += sum(1 for x in fn.insts if x.mfma and x.inline)
            for f in L.check_function(fn):
                report.append("%s [%s] %s" % (unit, L.template_name(fn.name) or fn.name, f.format()))
    assert n_inline > 0, "no inline MFMA found: the lint would check nothing"
    assert not report, "\n".join(report)


_SCAN_KERNELS = ("dense_scan_kernel", "dense_wide_scan_kernel", "dense8_scan_kernel", "dense8_scan_mt_kernel",
                 "dense8_body_kernel")


def test_every_scan_kernel_instantiation_has_a_variant_test(shipped_asm):
    from tests.test_hip_scan_variants import SCAN_VARIANTS
    names = set()
    for sym in L.function_names(shipped_asm["sq_dense.hip"]):
        t = L.template_name(sym)
        if t is not None and t.split("<")[0] in _SCAN_KERNELS:
            names.add(t)
    assert len(names) >= 70, sorted(names)
    missing = sorted(names - set(SCAN_VARIANTS))
    assert not missing, "scan kernels without an entry in tests/test_hip_scan_variants.py SCAN_VARIANTS: %s" % missing
    stale = sorted(set(SCAN_VARIANTS) - names)
    assert not stale, "SCAN_VARIANTS entries no longer compiled: %s" % stale


def test_template_names_of_mangled_symbols():
    assert L.template_name("_ZN2sq17dense_scan_kernelILi4ELi4ELi1ELi4ELi1ELb1ELb0ELb1EEEvNS_13DenseScanArgsE") == \
        "dense_scan_kernel<4,4,1,4,1,true,false,true>"
    assert L.template_name("_ZN2sq18dense8_body_kernelILi16ELb1EEEvNS_14Dense8ScanArgsENS_14Dense8TailArgsE") == \
        "dense8_body_kernel<16,true>"
    assert L.template_name("_ZN2sqL15fill_u32_kernelEPjxj") is None
    assert re.match(r"^\w+<", L.template_name("_ZN2sq22dense_wide_scan_kernelILi2ELi4ELb0EEEvNS_13DenseScanArgsEi"))
