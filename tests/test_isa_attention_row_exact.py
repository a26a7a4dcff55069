"""ISA check of the MFMA attention backward's single-row mode (attn_bwd_kernel<NQB, PERSIST, Q8,
ROW = true>, csrc/attention.hip; CPU: hipcc cross-compiles to gfx950 assembly, as
tests/test_isa_attention_row.py does).

The ROW instances exist for NQB = 1 .. 8 in both storage builds, and none spills more than the
full instance of the same NQB (NQB = 8 has no full instance — its dS^T does not fit the LDS — and
is held to the NQB = 7 one's figure): the mode removes work from the kernel, it must not add
scratch traffic to it."""
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
    out = tmp_path_factory.mktemp("isa_attn_rx") / f"attention_{request.param}.s"
    extra = ["-DLC_F16", "-include", os.path.join(CSRC, "lc_f16_names.h")] if request.param == "f16" else []
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-honor-nans",
                    f"-I{os.path.join(ROOT, 'include')}", "--cuda-device-only", "-S", *extra,
                    os.path.join(CSRC, "attention.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    return out.read_text()


def scratch_of(asm, nqb, row):
    """ScratchSize of attn_bwd_kernel<nqb, nqb >= 5, false, row>, None if not instantiated."""
    name = f"attn_bwd_kernelILi{nqb}ELb{int(nqb >= 5)}ELb0ELb{int(row)}EE"
    m = re.search(rf"^(_ZN12_GLOBAL__N_1\d+{name}\w*):", asm, re.M)
    if not m:
        return None
    end = asm.index(".Lfunc_end", m.end())
    scratch = re.search(r"; ScratchSize: (\d+)", asm[end:end + 4000])
    assert scratch, name
    return int(scratch.group(1))


def test_row_instances_exist_and_spill_no_more_than_the_full_ones(attention_asm):
    for nqb in range(1, 9):
        row = scratch_of(attention_asm, nqb, True)
        full = scratch_of(attention_asm, min(nqb, 7), False)
        assert row is not None, f"no ROW instance for NQB = {nqb}"
        assert full is not None, f"no full instance for NQB = {min(nqb, 7)}"
        print(f"attn_bwd_kernel NQB={nqb}: ScratchSize ROW {row} full {full}")
        assert row <= full, (nqb, row, full)
