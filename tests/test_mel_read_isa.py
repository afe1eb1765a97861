"""The shipped ISA of the kernels built from the front-end's device code, after
the power rows got an even pitch (CPU test on the built library):

  - the mel's power reads are single ds_read_b64, at least as many as the
    generator emitted 8-byte reads for the kernel's mode (csrc/wk_tables.h
    states the count per mode); they were ds_read2_b32 / ds_read_b32 pairs,
    153-161 + 6 per kernel, and none of those is left in the mel;
  - the compiler did not join them into ds_read2_b64: that form is still
    exactly the 8 reads of the two half-transposes;
  - the fp32 fused kernel fetches its weight fragments 16 bytes per lane:
    buffer_load_dwordx4 appears (25 fragment groups + 4 x 3 DCT operand loads)
    and buffer_load_dword falls (170 in the parent's fp32-audio kernel)."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "esp32-wake-word_amd", "csrc")
OPS = ("ds_read_b64", "ds_read2_b64", "ds_read2_b32", "buffer_load_dword", "buffer_load_dwordx4")
PARENT_FP32_DWORD_LOADS = {"float": 170, "short": 188}   # wk_fused_kernel<T, 0, *> before the 16-byte fragment loads


def mel_reads() -> dict:
    with open(os.path.join(CSRC, "wk_tables.h")) as fh:
        text = fh.read()
    out = {}
    for mode in "BA":
        m = re.search(rf"// mel{mode}: 8-byte power reads per wave \[[0-9, ]+\], (\d+) in all", text)
        out[mode] = int(m.group(1))
        assert out[mode] == sum(body.count("= q[") for body in re.findall(rf"(?s)void mel{mode}_w\d\(.*?\n\}}", text))
    return out


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa_rules
    from wakeword import _lib
    objdump = os.path.join(isa_rules.LLVM_BIN, "llvm-objdump")
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not found")
    assert os.path.exists(_lib.LIB_PATH), "build libwakeword.so first (python -m wakeword.build)"
    tmp = tmp_path_factory.mktemp("co")
    raw = {}
    for i, co in enumerate(isa_rules.code_objects(_lib.LIB_PATH)):
        f = str(tmp / f"co{i}.elf")
        with open(f, "wb") as fh:
            fh.write(co)
        cur = None
        for line in subprocess.run([objdump, "-d", "--mcpu=gfx950", f], capture_output=True, text=True,
                                   check=True).stdout.splitlines():
            m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
            if m:
                cur = m.group(1)
                continue
            t = line.split()
            if cur and t and t[0] in OPS:
                raw.setdefault(cur, dict.fromkeys(OPS, 0))[t[0]] += 1
    names = isa_rules._demangle(list(raw))
    fe = {names[k]: v for k, v in raw.items()
          if re.search(r"wk_fused_kernel|wk_frontend_kernel|wk_scan_frames_kernel|wk_scan_assemble_kernel", k)}
    assert len(fe) >= 12 + 4 + 2 + 2, sorted(fe)
    return fe


def test_mel_reads_are_single_8_byte_reads(counts):
    want = mel_reads()
    assert want["B"] >= 150 and want["A"] >= 150
    for k, v in counts.items():
        mode = "A" if "wk_frontend_kernel<false" in k else "B"
        print(k[:70], v)
        assert v["ds_read_b64"] >= want[mode], (k, v, want[mode])
        assert v["ds_read2_b64"] == 8, (k, v)
        assert v["ds_read2_b32"] <= (8 if "wk_fused_kernel" in k else 0), (k, v)   # (fused: the CNN role's, as before)


def test_fp32_fragments_are_16_byte_loads(counts):
    seen = 0
    for k, v in counts.items():
        m = re.search(r"wk_fused_kernel<(float|short), 0, (true|false)>", k)
        if not m:
            continue
        seen += 1
        assert v["buffer_load_dwordx4"] >= 25 + 12, (k, v)
        assert v["buffer_load_dword"] <= PARENT_FP32_DWORD_LOADS[m.group(1)] - 100, (k, v)
    assert seen == 4
