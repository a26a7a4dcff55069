"""ISA check of the single-query-row attention kernels (CPU: hipcc cross-compiles attention.hip to
gfx950 assembly, as tests/test_isa.py does for peft.hip and gemm.hip).

attn_row_bwd_kernel holds a lane's 16 K / V chunks (64 VGPRs) in registers from the first
instruction on so that every load is in flight before the first use; a spill would turn that into
scratch traffic and serialise the loads behind vmcnt(0). Both storage builds keep ScratchSize 0
and stay at or under 128 VGPRs. The single-row instances of the forward (attn_fwd_kernel<NQB,
ONLINE, ROW = true>) must not spill either, like the full ones."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lifelong-clip_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module", params=["bf16", "f16"])
def attention_asm(request, tmp_path_factory):
    if not os.path.exists(HIPCC) or shutil.which("make") is None:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_attn") / f"attention_{request.param}.s"
    extra = ["-DLC_F16", "-include", os.path.join(CSRC, "lc_f16_names.h")] if request.param == "f16" else []
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-honor-nans",
                    f"-I{os.path.join(ROOT, 'include')}", "--cuda-device-only", "-S", *extra,
                    os.path.join(CSRC, "attention.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    return out.read_text()


def test_row_forward_instances_do_not_spill(attention_asm):
    found = 0
    for m in re.finditer(r"^(_ZN12_GLOBAL__N_115attn_fwd_kernelILi\d+ELb[01]ELb1EE\w*):",
                         attention_asm, re.M):
        end = attention_asm.index(".Lfunc_end", m.end())
        scratch = re.search(r"; ScratchSize: (\d+)", attention_asm[end:end + 4000])
        assert scratch and int(scratch.group(1)) == 0, f"{m.group(1)} spills"
        found += 1
    assert found == 16, found  # NQB = 1..8, online and two-pass


def test_row_backward_does_not_spill(attention_asm):
    kernel = "attn_row_bwd_kernel"
    m = re.search(rf"^(_ZN12_GLOBAL__N_1\d+{kernel}E\w*):", attention_asm, re.M)
    assert m, f"{kernel} not found in the assembly"
    end = attention_asm.index(".Lfunc_end", m.end())
    tail = attention_asm[end:end + 4000]
    scratch = re.search(r"; ScratchSize: (\d+)", tail)
    vgprs = re.search(r"; NumVgprs: (\d+)", tail)
    assert scratch and int(scratch.group(1)) == 0, f"{kernel} spills: {scratch and scratch.group(0)}"
    assert vgprs and int(vgprs.group(1)) <= 128, f"{kernel}: {vgprs and vgprs.group(0)}"
