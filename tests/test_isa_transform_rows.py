"""ISA check of the padded patch-row transform kernels (CPU: hipcc cross-compiles transform.hip to
gfx950 assembly, as tests/test_isa_attention_long.py does).

train_transform_rows_sep_kernel keeps four column pairs' decode (channel, ky, kx, 1/std, -mean/std)
per lane across its patch walk, and train_transform_rows_kernel selects the per-channel constants
by a lane-varying channel; a runtime-indexed copy of either would live in scratch. Both keep
ScratchSize 0. Only that figure and the kernel names are read."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lifelong-clip_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def transform_asm(tmp_path_factory):
    if not os.path.exists(HIPCC) or shutil.which("make") is None:
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa_transform_rows") / "transform.s"
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17",
                    f"-I{os.path.join(ROOT, 'include')}", "--cuda-device-only", "-S",
                    os.path.join(CSRC, "transform.hip"), "-o", str(out)],
                   check=True, capture_output=True)
    return out.read_text()


@pytest.mark.parametrize("kernel", ["train_transform_rows_sep_kernel",
                                    "train_transform_rows_kernel"])
def test_rows_kernels_do_not_spill(transform_asm, kernel):
    found = re.findall(rf"^(_ZN12_GLOBAL__N_1\d+{kernel}E\w*):", transform_asm, re.M)
    assert len(found) == 1, found
    start = transform_asm.index(found[0] + ":")
    end = transform_asm.index(".Lfunc_end", start)
    scratch = re.search(r"; ScratchSize: (\d+)", transform_asm[end:end + 4000])
    assert scratch and int(scratch.group(1)) == 0, f"{found[0]} spills"
