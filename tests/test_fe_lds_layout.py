"""The front-end's LDS table layout (csrc/wk_fe_lds_layout.h), checked on the
host: a small C++ program is compiled against the header and

  - maps every (lane, slot) of every table to a distinct in-range offset;
  - checks that every 16-byte read (two adjacent entries) is 16-byte aligned;
  - under the LDS banking of the 8- and 16-byte reads, bank = (byte address / 4)
    mod 64, checks that the 16 distinct j of each lane group land on 16
    distinct bank quads (ds_read_b128: four groups of 16 lanes) and, for a
    single entry read as 8 bytes, on 16 distinct bank pairs (ds_read_b64: two
    halves of 32 lanes; lanes sharing a j share an address and broadcast);
  - checks the transpose scratch: written cells distinct and inside the row,
    every read cell written, each frame group's 16 lanes on 16 distinct bank
    pairs (and prints how many pairs the two groups of a 32-lane half share:
    8, which is why the transposes' reads stay ds_read2_b64);
  - restates fe_init_tables through the index functions and finds, value for
    value, W256^(j (s ^ (j & 8))), fe_split_tw(j, k2) and the sign-adjusted
    window where the slot-major layout held them;
  - checks both carve sizes against their limits.

The program prints one line per failed check and exits non-zero."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "esp32-wake-word_amd", "csrc")

PROGRAM = r"""
#include <cmath>
#include <cstdio>
#include <set>
#include <vector>
#include "wk_fe_lds_layout.h"
using namespace wk::fe_lds;

// ds_read_b128 lane groups (MI355X): lanes served in one LDS cycle
static const int kGroups128[4][16] = {
    {0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31},
    {32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59},
    {36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63}};

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { ++fails; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

// the former slot-major tables and the device formulas (host double -> float; the comparison is about placement)
static void w256(int j, int s, float* o) {
  const int k1 = s ^ (j & 8);
  o[0] = (float)std::cos(-M_PI * (j * k1) / 128.0);
  o[1] = (float)std::sin(-M_PI * (j * k1) / 128.0);
}
static bool split_flip(int j, int k2) { return j == 8 || (j >= 1 && j <= 7 && !(k2 & 1)) || (j >= 9 && (k2 & 1)); }
static void split_tw(int j, int k2, float* o) {
  const float cs = (float)std::cos(-M_PI * (j + 16 * k2) / 256.0), sn = (float)std::sin(-M_PI * (j + 16 * k2) / 256.0);
  o[0] = split_flip(j, k2) ? -cs : cs;
  o[1] = sn;
}

int main(int argc, char** argv) {
  const int lstride = 64, n_frames = 63, p_row = 271;
  std::vector<float> win_const(320);
  if (argc > 1) {   // the constant window table, one value per line
    std::FILE* fh = std::fopen(argv[1], "r");
    for (int i = 0; i < 320; ++i) CHECK(fh && std::fscanf(fh, "%f", &win_const[i]) == 1, "window value %d", i);
    if (fh) std::fclose(fh);
  }

  // 1. distinct, in-range offsets; 16-byte aligned reads
  {
    std::set<int> seen;
    for (int j = 0; j < kLanes; ++j) {
      CHECK(row_off(j) % 4 == 0, "row_off(%d) alignment", j);
      for (int s = 0; s < kTwSlots; ++s)
        for (int c = 0; c < 2; ++c) {
          const int o = tw_off(j, s) + c;
          CHECK(o >= 0 && o < kTabSize && seen.insert(o).second, "tw_off(%d,%d)+%d = %d", j, s, c, o);
        }
      for (int k2 = 0; k2 < kSplitSlots; ++k2)
        for (int c = 0; c < 2; ++c) {
          const int o = split_off(j, k2) + c;
          CHECK(o >= 0 && o < kTabSize && seen.insert(o).second, "split_off(%d,%d)+%d = %d", j, k2, c, o);
        }
      for (int s = 0; s < kTwSlots; s += 2)
        CHECK(tw_off(j, s) % 4 == 0 && tw_off(j, s + 1) == tw_off(j, s) + 2, "tw pair (%d,%d)", j, s);
      for (int k2 = 0; k2 < kSplitSlots; k2 += 2)
        CHECK(split_off(j, k2) % 4 == 0 && split_off(j, k2 + 1) == split_off(j, k2) + 2, "split pair (%d,%d)", j, k2);
    }
    CHECK((int)seen.size() == kLanes * kRowUsed, "twiddle rows hold %d floats", (int)seen.size());
    std::set<int> wseen;
    for (int j = 0; j < kLanes; ++j)
      for (int n1 = 0; n1 < kWinRows; ++n1) {
        for (int c = 0; c < 2; ++c) {
          const int o = win_off(j, n1) + c;
          CHECK(o >= 0 && o < kWinSize && wseen.insert(o).second, "win_off(%d,%d)+%d = %d", j, n1, c, o);
        }
        if (n1 % 2 == 0)
          CHECK(win_off(j, n1) % 4 == 0 && win_off(j, n1 + 1) == win_off(j, n1) + 2, "win pair (%d,%d)", j, n1);
      }
    CHECK((int)wseen.size() == 320, "window rows hold %d floats", (int)wseen.size());
  }

  // 2. banking.  Lane l holds j = l & 15; every table base in the carve is 16-byte aligned.
  const Carve cv = carve(lstride, n_frames, p_row);
  CHECK(cv.tab % 4 == 0 && cv.win % 4 == 0 && cv.logmel % 4 == 0 && cv.power % 2 == 0, "carve alignment");
  auto check128 = [&](const char* what, int base, int (*off)(int, int), int slot) {
    for (int g = 0; g < 4; ++g) {
      std::set<int> quads, js;
      for (int i = 0; i < 16; ++i) {
        const int j = kGroups128[g][i] & 15;
        js.insert(j);
        const int a = base + off(j, slot);
        CHECK(a % 4 == 0, "%s slot %d lane j %d: float offset %d not 16-byte aligned", what, slot, j, a);
        quads.insert((a % 64) / 4);
      }
      CHECK(js.size() == 16 && quads.size() == 16, "%s slot %d group %d: %d j on %d bank quads", what, slot, g,
            (int)js.size(), (int)quads.size());
    }
  };
  for (int s = 0; s < kTwSlots; s += 2) check128("tw", cv.tab, tw_off, s);
  for (int k2 = 0; k2 < kSplitSlots; k2 += 2) check128("split", cv.tab, split_off, k2);
  for (int n1 = 0; n1 < kWinRows; n1 += 2) check128("win", cv.win, win_off, n1);
  // a single table entry read as 8 bytes (ds_read_b64: two halves of 32 lanes,
  // each j twice at one address): the 16 j on 16 distinct bank pairs
  auto check64 = [&](const char* what, int base, int (*off)(int, int), int slot) {
    for (int half = 0; half < 2; ++half) {
      std::set<int> pairs, addrs;
      for (int l = 32 * half; l < 32 * half + 32; ++l) {
        const int a = base + off(l & 15, slot);
        CHECK(a % 2 == 0, "%s slot %d: 8-byte alignment", what, slot);
        addrs.insert(a);
        pairs.insert((a % 64) / 2);
      }
      CHECK(addrs.size() == 16 && pairs.size() == 16, "%s slot %d half %d: %d addresses on %d bank pairs", what, slot,
            half, (int)addrs.size(), (int)pairs.size());
    }
  };
  for (int s = 0; s < kTwSlots; ++s) check64("tw", cv.tab, tw_off, s);
  for (int k2 = 0; k2 < kSplitSlots; ++k2) check64("split", cv.tab, split_off, k2);
  for (int n1 = 0; n1 < kWinRows; ++n1) check64("win", cv.win, win_off, n1);
  // The transposes' 8-byte reads (not a table: every lane its own address).
  // A frame group's 16 lanes sit on 16 distinct bank pairs.  As single
  // ds_read_b64 a 32-lane half also holds the group 16 rows further on, whose
  // scratch starts 16 * 271 = 48 mod 64 floats later: 8 of its 16 bank pairs
  // are the first group's (2-way), which the row pitch fixes -- printed, not
  // required (the pair form, ds_read2_b64, serves 16 contiguous lanes at a time).
  int worst = 0;
  for (int fl = 0; fl < 16; ++fl)
    for (int pass = 0; pass < 2; ++pass)
      for (int s = 0; s < 8; ++s) {
        std::set<int> both;
        for (int grp = 0; grp < 2; ++grp) {
          const int f = fl + 16 * grp, xs = cv.power + f * p_row + (f & 1);
          CHECK(xs % 2 == 0, "scratch of row %d not 8-byte aligned", f);
          std::set<int> pairs;
          for (int j = 0; j < 16; ++j) {
            const int a = xs + 2 * xpose_rd(pass ? j ^ 8 : j, s);
            CHECK(a + 1 < cv.power + f * p_row + p_row, "transpose read outside row %d", f);
            pairs.insert((a % 64) / 2);
            both.insert((a % 64) / 2);
          }
          CHECK(pairs.size() == 16, "transpose read s %d pass %d row %d: 16 lanes on %d bank pairs", s, pass, f,
                (int)pairs.size());
        }
        if (32 - (int)both.size() > worst) worst = 32 - (int)both.size();
      }
  std::printf("transpose_b64_shared_pairs_per_half %d\n", worst);
  {
    std::set<int> cells;   // the transpose image: distinct cells inside the scratch
    for (int j = 0; j < 16; ++j)
      for (int s = 0; s < 8; ++s) {
        const int w = xpose_wr(j) + s;
        CHECK(w >= 0 && 2 * w + 1 < kXposeFloats && cells.insert(w).second, "xpose_wr(%d)+%d", j, s);
      }
    for (int kc = 0; kc < 16; ++kc)
      for (int s = 0; s < 8; ++s) CHECK(cells.count(xpose_rd(kc, s)) == 1, "xpose_rd(%d,%d) reads no written cell", kc, s);
    CHECK(kXposeFloats <= p_row - 1, "scratch fits the row");
  }

  // 3. fe_init_tables restated through the index functions vs the slot-major tables
  {
    std::vector<float> old_tw(16 * 16 * 2), old_tws(7 * 16 * 2), old_w0(16 * 2);
    for (int i = 0; i < 256; ++i) w256(i % 16, i / 16, &old_tw[2 * i]);
    for (int i = 0; i < 7 * 16; ++i) split_tw(i % 16, i / 16 + 1, &old_tws[2 * i]);
    for (int j = 0; j < 16; ++j) split_tw(j, 0, &old_w0[2 * j]);
    std::vector<float> smem(cv.end, -7.0f);
    for (int i = 0; i < 320; ++i) {
      const int n1 = i / 32, jj = (i % 32) / 2, c = i & 1;
      CHECK(win_src(jj, n1) + c == i, "win_src(%d,%d)", jj, n1);
      smem[cv.win + win_off(jj, n1) + c] = win_const[i];
    }
    for (int i = 0; i < 256; ++i) w256(i % 16, i / 16, &smem[cv.tab + tw_off(i % 16, i / 16)]);
    for (int i = 0; i < 8 * 16; ++i) split_tw(i % 16, i / 16, &smem[cv.tab + split_off(i % 16, i / 16)]);
    for (int j = 0; j < 16; ++j) {
      for (int s = 0; s < 16; ++s)
        for (int c = 0; c < 2; ++c)
          CHECK(smem[cv.tab + tw_off(j, s) + c] == old_tw[(s * 16 + j) * 2 + c], "W256 value (%d,%d)", j, s);
      for (int k2 = 0; k2 < 8; ++k2)
        for (int c = 0; c < 2; ++c) {
          const float want = k2 == 0 ? old_w0[2 * j + c] : old_tws[((k2 - 1) * 16 + j) * 2 + c];
          CHECK(smem[cv.tab + split_off(j, k2) + c] == want, "split value (%d,%d)", j, k2);
        }
      for (int n1 = 0; n1 < 10; ++n1)
        for (int c = 0; c < 2; ++c)
          CHECK(smem[cv.win + win_off(j, n1) + c] == win_const[32 * n1 + 2 * j + c], "window value (%d,%d)", j, n1);
    }
  }

  // 4. carve sizes
  CHECK(cv.end_no_win * 4 <= kStandaloneLimitBytes, "standalone carve %d B", cv.end_no_win * 4);
  CHECK(cv.end * 4 <= kFusedLimitBytes, "front-end part of the fused carve %d B", cv.end * 4);
  std::printf("standalone_bytes %d fused_fe_bytes %d tab_floats %d\n", cv.end_no_win * 4, cv.end * 4, kTabSize);
  return fails ? 1 : 0;
}
"""


def _window_table():
    """kWinB of csrc/wk_tables.h (sign-adjusted Hamming window), as the device holds it."""
    with open(os.path.join(CSRC, "wk_tables.h")) as fh:
        m = re.search(r"kWinB\[320\] = \{([^}]*)\}", fh.read())
    vals = [v.strip().rstrip("f") for v in m.group(1).split(",")]
    assert len(vals) == 320
    return vals


def test_fe_lds_layout(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    src = tmp_path / "layout_check.cpp"
    src.write_text(PROGRAM)
    win = tmp_path / "win.txt"
    win.write_text("\n".join(_window_table()) + "\n")
    exe = tmp_path / "layout_check"
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I", CSRC, str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe), str(win)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "FAIL" not in r.stdout, r.stdout
    m = re.search(r"standalone_bytes (\d+) fused_fe_bytes (\d+) tab_floats (\d+)", r.stdout)
    assert m and int(m.group(1)) <= 81920 and int(m.group(3)) == 832


def test_table_reads_are_16_byte_reads_in_the_shipped_isa(tmp_path):
    """Every kernel built from the front-end's device code: its only ds_read2_b64
    are the 8 reads of the two half-transposes (a slot-major table read compiles
    to that pair form; the parent had 24 in the fused kernels, 19 in the others),
    and the 12 twiddle-row reads (+ 5 window reads, fused) are ds_read_b128."""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa_rules
    from wakeword import _lib
    objdump = os.path.join(isa_rules.LLVM_BIN, "llvm-objdump")
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not found")
    assert os.path.exists(_lib.LIB_PATH), "build libwakeword.so first (python -m wakeword.build)"
    counts = {}
    for i, co in enumerate(isa_rules.code_objects(_lib.LIB_PATH)):
        f = str(tmp_path / f"co{i}.elf")
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
            if cur and t and t[0] in ("ds_read2_b64", "ds_read_b128"):
                counts.setdefault(cur, {"ds_read2_b64": 0, "ds_read_b128": 0})[t[0]] += 1
    fe = {k: v for k, v in counts.items()
          if re.search(r"wk_fused_kernel|wk_frontend_kernel|wk_scan_frames_kernel|wk_scan_assemble_kernel", k)}
    assert len(fe) >= 12 + 4 + 2 + 2, sorted(fe)   # fused: 2 audio types x 3 precisions x feats; front-end 2 x 2; scan 2 + 2
    for k, v in fe.items():
        fused = "wk_fused_kernel" in k
        assert v["ds_read2_b64"] == 8, (k, v)
        assert v["ds_read_b128"] >= (17 if fused else 12), (k, v)


def test_fused_carve_within_budget():
    """The fused kernel's whole carve is a static_assert in wk_fused_lds.h; here: the
    device header derives its offsets from the layout header's carve()."""
    with open(os.path.join(CSRC, "wk_fe_dev.h")) as fh:
        dev = fh.read()
    assert "fe_lds::carve(WK_LSTRIDE, kNFramesB, kPRow)" in dev
    with open(os.path.join(CSRC, "wk_fused_lds.h")) as fh:
        assert "static_assert(kFusedLds * 4 <= 163840" in fh.read()
