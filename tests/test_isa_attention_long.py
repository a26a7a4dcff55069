"""ISA check of the long attention family (257..512 tokens; CPU: hipcc cross-compiles
attention.hip to gfx950 assembly, as tests/test_isa_attention_row.py does).

attn_long_fwd_kernel / attn_long_bwd_kv_kernel / attn_long_bwd_q_kernel<NCH>, NCH = 9..16: a wave
walks two chunks with the per-chunk bodies of the one-wave-per-chunk kernels, and stages up to 8
passes of row pieces through registers. A spill would put scratch traffic inside the key / query
sweeps; both storage builds keep ScratchSize 0 in every instance. Only that figure and the kernel
names are read."""
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
    out = tmp_path_factory.mktemp("isa_attn_long") / f"attention_{request.param}.s"
    extra = ["-DLC_F16", "-include", os.path.join(CSRC, "lc_f16_names.h")] if request.param == "f16" else []
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-honor-nans",
                    f"-I{os.path.join(ROOT, 'include')}", "--cuda-device-only", "-S", *extra,
                    os.path.join(CSRC, "attention.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    return out.read_text()


@pytest.mark.parametrize("kernel", ["attn_long_fwd_kernel", "attn_long_bwd_kv_kernel",
                                    "attn_long_bwd_q_kernel"])
def test_long_instances_do_not_spill(attention_asm, kernel):
    chunks = []
    for m in re.finditer(rf"^(_ZN12_GLOBAL__N_1\d+{kernel}ILi(\d+)EE\w*):", attention_asm, re.M):
        end = attention_asm.index(".Lfunc_end", m.end())
        scratch = re.search(r"; ScratchSize: (\d+)", attention_asm[end:end + 4000])
        assert scratch and int(scratch.group(1)) == 0, f"{m.group(1)} spills"
        chunks.append(int(m.group(2)))
    assert sorted(chunks) == list(range(9, 17)), chunks  # NCH = 9..16, nothing else
