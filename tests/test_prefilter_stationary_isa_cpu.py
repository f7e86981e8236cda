"""The register budget gmm_prefilter_stationary_kernel's launch geometry rests on, read from the gfx950 code object without a GPU
(tools/isa_info.py): 256 threads, two workgroups per CU = two waves per SIMD = at most 256 vector registers (VGPRs + AGPRs) per
lane, the group's A operand (32 registers per k-step) among them, and no scratch: a spilled A fragment would be reloaded for
every 16-frame block.  The kernel has no LDS and no barrier either: its waves share nothing but the caches."""
import os
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_info  # noqa: E402

pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(isa_info.LLVM, "llvm-objdump")), reason="no ROCm LLVM tools")

KERNELS = ["gmm_prefilter_stationary_kernel<1>", "gmm_prefilter_stationary_kernel<2>", "gmm_prefilter_stationary_kernel<3>"]


@pytest.fixture(scope="module")
def prefilter_object():
    from speechrecognition_amd import build
    build.build()
    with tempfile.TemporaryDirectory() as tmp:
        co = isa_info.code_object("gmm_prefilter", tmp)
        yield isa_info.kernel_metadata(co), isa_info.disassembly(co)


@pytest.mark.parametrize("kernel", KERNELS)
def test_two_waves_per_simd_without_scratch(prefilter_object, kernel):
    md, _ = prefilter_object
    assert kernel in md, sorted(md)
    k = md[kernel]
    assert k["vgpr_count"] + k.get("agpr_count", 0) <= 256, k
    assert k["private_segment_fixed_size"] == 0 and k.get("vgpr_spill_count", 0) == 0 and k.get("sgpr_spill_count", 0) == 0, k


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_lds_and_no_barrier(prefilter_object, kernel):
    md, dis = prefilter_object
    assert md[kernel]["group_segment_fixed_size"] == 0
    ops = [x.split()[0] for x in dis[kernel]]
    assert "s_barrier" not in ops and not any(o.startswith("ds_read") or o.startswith("ds_write") for o in ops)
    # per step: 2 blocks x 8 row blocks x KS32 matrix instructions, twice (the frame loop is unrolled over its two operand buffers)
    ks32 = int(kernel[-2])
    assert sum(o.startswith("v_mfma_f32_16x16x32") for o in ops) == 2 * 2 * 8 * ks32


def _early_reads_of_mfma_results(insts, need=11):
    """(mfma, reader, wait states) for every inline-asm epilogue instruction (v_min3_f32, v_cmp_ngt_f32) that reads an MFMA's
    destination fewer than `need` wait states behind it.  The compiler pads the hazards of instructions it emits itself, but it does
    not look into inline asm; an 8-pass MFMA result needs 11 wait states before a VALU instruction may read it (an instruction
    counts one, `s_nop N` counts N + 1: the compiler's own conservative count)."""
    import re
    out = []
    for i, x in enumerate(insts):
        m = re.match(r"v_mfma\S+ v\[(\d+):(\d+)\]", x)
        if not m:
            continue
        lo, hi = int(m.group(1)), int(m.group(2))
        ws = 0
        for y in insts[i + 1:]:
            if ws >= need:
                break
            if y.startswith(("s_cbranch", "s_branch", "s_endpgm")):
                break  # (the loop's back edge lands on MFMAs and loads, never on the epilogue)
            if y.startswith(("v_min3_f32", "v_cmp_ngt_f32")) and any(lo <= int(r) <= hi for r in re.findall(r"v(\d+)", y.split(None, 1)[1])):
                out.append((x, y, ws))
                break
            ws += int(y.split()[1], 0) + 1 if y.startswith("s_nop") else 1
    return out


@pytest.mark.parametrize("kernel", KERNELS + ["gmm_prefilter16_kernel<3, 4>"])
def test_the_asm_epilogue_reads_no_mfma_result_early(prefilter_object, kernel):
    """A first version of the stationary kernel had no fence between its MFMAs and its epilogue: the compiler moved v_min3_f32 up to
    two instructions behind the MFMA whose result it reads, and every mask came out empty."""
    _, dis = prefilter_object
    assert _early_reads_of_mfma_results(dis[kernel]) == []


def test_the_early_read_check_sees_one():
    insts = ["v_mfma_f32_16x16x32_f16 v[152:155], v[8:11], v[100:103], v[120:123]", "s_nop 1", "v_add_co_u32_e32 v120, vcc, s11, v104",
             "v_min3_f32 v188, v188, v152, v153"]
    assert [w for _, _, w in _early_reads_of_mfma_results(insts)] == [3]
    assert _early_reads_of_mfma_results(insts[:1] + ["s_nop 7", "s_nop 2"] + insts[3:]) == []
