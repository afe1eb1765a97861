"""The even power-row pitch and what rests on it (csrc/wk_common.h kPRow,
csrc/wk_fe_lds_layout.h, the mel functions of csrc/wk_tables.h), checked on the
host.  A small C++ program compiled against the layout header enumerates

  - the mel's lane-per-frame 8-byte reads {p[2m], p[2m+1]} (ds_read_b64: two
    halves of 32 lanes, bank = dword address mod 64): per half 32 lanes on 32
    distinct bank pairs, every address 8-byte aligned and inside its row;
  - the power-row stores of the FFT phase under the frame-slot mapping
    (ds_write_b32 / ds_write2_b32: two halves of 32 lanes, bank = dword address
    mod 32): the two 16-lane frame groups of a half on disjoint banks, for the
    low bins j + 16 k2 and the high bins 256 - j - 16 k2;
  - the frame-slot mapping: a bijection onto slots 0..63 with frame 0 in wave 0 /
    round 0 / group 0, frame 62 in wave 6 / round 1 / group 3 and the padding
    slot 63 in wave 7 / round 1 / group 3 (the lanes the edge paths assume);
  - the transpose scratch inside the row, and both LDS budgets.

From wk_tables.h, per mode and filter: the (bin, weight) sequence of the FMA
chain equals the generator's filterbank in ascending bin order (what keeps the
log-mel bit-identical whatever the read form), every read is a pair index
inside the row, and nnz is the 493 / 454 the header states."""
import importlib.util
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "esp32-wake-word_amd")
CSRC = os.path.join(PKG, "csrc")

PROGRAM = r"""
#include <cstdio>
#include <set>
#include "wk_fe_lds_layout.h"
using namespace wk::fe_lds;

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

int main() {
  const int lstride = 64, n_frames = 63, p_row = P_ROW;
  const Carve cv = carve(lstride, n_frames, p_row);

  // 1. the mel's reads: lane l reads the pair m of row min(l, 62)
  CHECK(p_row % 2 == 0 && cv.power % 2 == 0, "rows 8-byte aligned");
  CHECK(mel_rows_conflict_free(p_row), "mel_rows_conflict_free(%d)", p_row);
  for (int m = 0; m <= 128; ++m)
    for (int half = 0; half < 2; ++half) {
      std::set<int> pairs, addrs;
      for (int l = 32 * half; l < 32 * half + 32; ++l) {
        const int row = l < n_frames ? l : n_frames - 1, a = cv.power + row * p_row + 2 * m;
        CHECK(a % 2 == 0, "pair %d lane %d: float offset %d not 8-byte aligned", m, l, a);
        CHECK(2 * m + 1 < p_row && a + 1 < cv.power + (row + 1) * p_row && a + 1 < cv.end_no_win,
              "pair %d lane %d outside its row", m, l);
        if (addrs.insert(a).second) pairs.insert((a % 64) / 2);   // equal addresses broadcast
      }
      CHECK(pairs.size() == addrs.size() && addrs.size() == (half ? 31u : 32u),
            "pair %d half %d: %d addresses on %d bank pairs", m, half, (int)addrs.size(), (int)pairs.size());
    }

  // 2. the frame-slot mapping
  {
    std::set<int> slots;
    for (int w = 0; w < 8; ++w)
      for (int r = 0; r < 2; ++r)
        for (int g = 0; g < 4; ++g) {
          const int fl = frame_slot(w, r, g);
          CHECK(fl >= 0 && fl < 64 && slots.insert(fl).second, "frame_slot(%d,%d,%d) = %d", w, r, g, fl);
          CHECK(fl == w + kRoundSlots * r + slot_base(g), "frame_slot is wave + round + group base");
        }
    CHECK(slots.size() == 64, "bijection onto 0..63");
    CHECK(frame_slot(0, 0, 0) == 0, "frame 0 in wave 0 / round 0 / group 0");
    CHECK(frame_slot(6, 1, 3) == 62, "frame 62 in wave 6 / round 1 / group 3");
    CHECK(frame_slot(7, 1, 3) == 63, "padding slot 63 in wave 7 / round 1 / group 3");
  }

  // 3. power-row stores: lane (g, j) stores row[j + 16 k2] and row[256 - j - 16 k2]
  // of its frame; a 32-lane half holds groups 2h and 2h + 1
  for (int w = 0; w < 8; ++w)
    for (int r = 0; r < 2; ++r)
      for (int half = 0; half < 2; ++half)
        for (int k2 = 0; k2 < 8; ++k2)
          for (int hi = 0; hi < 2; ++hi) {
            std::set<int> banks[2];
            for (int gg = 0; gg < 2; ++gg)
              for (int j = 0; j < 16; ++j) {
                const int fl = frame_slot(w, r, 2 * half + gg);
                const int bin = hi ? 256 - j - 16 * k2 : j + 16 * k2;
                CHECK(bin >= 0 && bin < p_row, "bin inside the row");
                banks[gg].insert((cv.power + fl * p_row + bin) % 32);
              }
            bool disjoint = banks[0].size() == 16 && banks[1].size() == 16;
            for (int b : banks[0]) disjoint = disjoint && !banks[1].count(b);
            CHECK(disjoint, "stores wave %d round %d half %d k2 %d %s: groups share banks", w, r, half, k2,
                  hi ? "high" : "low");
          }

  // 4. the transpose scratch is the row; budgets
  CHECK(kXposeFloats <= p_row, "scratch fits the row");
  for (int j = 0; j < 16; ++j)
    for (int s = 0; s < 8; ++s) CHECK(2 * (xpose_wr(j) + s) + 1 < p_row, "xpose_wr(%d)+%d inside the row", j, s);
  CHECK(cv.end_no_win * 4 <= kStandaloneLimitBytes, "standalone carve %d B", cv.end_no_win * 4);
  CHECK(cv.end * 4 <= kFusedLimitBytes, "front-end part of the fused carve %d B", cv.end * 4);
  std::printf("standalone_bytes %d fused_fe_bytes %d\n", cv.end_no_win * 4, cv.end * 4);
  return fails ? 1 : 0;
}
"""


def p_row() -> int:
    with open(os.path.join(CSRC, "wk_common.h")) as fh:
        return int(re.search(r"constexpr int kPRow = (\d+);", fh.read()).group(1))


def test_power_row_layout(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    assert p_row() == 270
    src = tmp_path / "power_row_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "power_row_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", f"-DP_ROW={p_row()}", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout
    m = re.search(r"standalone_bytes (\d+) fused_fe_bytes (\d+)", r.stdout)
    assert m and int(m.group(1)) <= 81920 and int(m.group(2)) <= 163840


def test_fused_budget_and_alignment_asserts_are_in_place():
    with open(os.path.join(CSRC, "wk_fe_dev.h")) as fh:
        dev = fh.read()
    assert "kPRow % 2 == 0" in dev and "fe_lds::mel_rows_conflict_free(kPRow)" in dev
    with open(os.path.join(CSRC, "wk_fused_lds.h")) as fh:
        assert "static_assert(kFusedLds * 4 <= 163840" in fh.read()
    with open(os.path.join(CSRC, "wk_fused_fe_role.h")) as fh:
        fe_role = fh.read()
    assert "fe_lds::slot_base(g)" in fe_role and "fe_lds::kRoundSlots * r" in fe_role


def mel_functions(text: str, name: str):
    """{wave: (pairs read [m], {bin: (pair, half)} of the register image, [(bin, filter, weight)] in source order)}."""
    out = {}
    for m in re.finditer(rf"void {name}_w(\d)\(const float\* __restrict__ row, float\* __restrict__ l\) \{{(.*?)\n\}}",
                         text, re.S):
        body = m.group(2)
        assert "assume_aligned(row, 8)" in body
        reads, image = [], {}
        for r, pair, rest in re.findall(r"const wk_mel_f2 r(\d+) = q\[(\d+)\];(.*)", body):
            assert r == pair
            reads.append(int(pair))
            for k, r2, h in re.findall(r"p\[(\d+)\] = r(\d+)\.([xy]);", rest):
                assert r2 == pair and int(k) == 2 * int(pair) + (h == "y") and int(k) not in image
                image[int(k)] = (int(pair), h)
        assert body.count("= q[") == len(reads) and body.count("] = r") == len(image)
        fmas = []
        for k, blk in re.findall(r"\{ const float v = p\[(\d+)\];(.*?)\}", body):
            assert int(k) in image, "a bin is used only after its pair was read"
            terms = re.findall(r"a(\d+) = __builtin_fmaf\(v, ([0-9.e+-]+)f, a(\d+)\);", blk)
            assert blk.count("__builtin_fmaf(") == len(terms) and all(f == f2 for f, _, f2 in terms)
            fmas += [(int(k), int(f), w) for f, w, _ in terms]
        assert body.count("__builtin_fmaf(") == len(fmas)
        assert body.index("{ const float v") > body.rindex("= q["), "all reads are issued before the first FMA"
        out[int(m.group(1))] = (reads, image, fmas)
    return out


@pytest.fixture(scope="module")
def gen():
    spec = importlib.util.spec_from_file_location("gen_tables", os.path.join(PKG, "tools", "gen_tables.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("mode", ["B", "A"])
def test_mel_chains_are_the_filterbank_in_ascending_bin_order(gen, mode):
    with open(os.path.join(CSRC, "wk_tables.h")) as fh:
        text = fh.read()
    fb, scale, nnz = (gen.fb_mode_b(), 0.25, 493) if mode == "B" else (gen.fb_mode_a(), 1.0, 454)
    assert f"nnz(mode {mode} fbank) = {nnz}" in text and int((fb != 0).sum()) == nnz
    waves = mel_functions(text, f"mel{mode}")
    assert sorted(waves) == list(range(8))
    got = {}
    n_reads = 0
    for w, (reads, image, fmas) in waves.items():
        n_reads += len(reads)
        assert len(set(reads)) == len(reads), "a pair is read once per wave"
        for pair in reads:
            assert 0 <= pair and 2 * pair + 1 < p_row()
        for k, f, wt in fmas:
            got.setdefault(f, []).append((k, np.float32(float(wt))))
    assert sorted(got) == list(range(40))
    total = 0
    for f in range(40):
        bins = np.nonzero(fb[:, f])[0]
        want = [(int(k), np.float32(np.float32(fb[k, f]) * np.float32(scale))) for k in bins]
        assert got[f] == want, (mode, f)
        total += len(want)
    assert total == nnz
    m = re.search(rf"// mel{mode}: 8-byte power reads per wave \[[0-9, ]+\], (\d+) in all", text)
    assert m and int(m.group(1)) == n_reads
