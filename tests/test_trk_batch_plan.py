"""CPU test of the open-loop tracking launches' plan (gnss-sdr-1_amd/csrc/trk_batch_plan.h): slices per job and LDS code window of a
batch launch, slices of a level-1 call, printed by tests/trk_batch_plan_selftest.cpp, against a table worked out by hand from the
rules (integer divisions round down):

  slices    forced (gc_trk_batch_set_slices > 0): that many.  Else jobs = channels * epochs, want = 8 * CUs (CUs <= 0: 256);
            jobs >= want: 1; else min(ceil(want / jobs), max((len + 511) / 512 / 4, 1), 64)
  window    the whole table unless len >= 4096, sizing is on (set_slices(-1) turns it off), the format is plain or complex float
            chips (not high-dynamics, not 16-bit) and the kernel has the small-window path.  Then, with l_max the longest code:
              plain chips, slices not forced, l_max + 64 > 4096 + 128: slices = max(slices, ceil(l_max / 4096))
              slices > 1: cps = ceil((len + 16 + 511) / 512 / slices) chunks per slice, chips per sample = max_step when the records
                are on the host, else l_max / len;
                need = words per chip * (ceil(cps * 512 * chips per sample * 1.002 + widest tap spread) + 64)
                need < table and table > 4096 + 128: window = max(need rounded up to 64, 1024); need is compared as a double, so a
                huge or non-finite step leaves the table whole
  level 1   N <= one_wg_max: 1; else max((N + 1 + 511) / 512 / 2, 1); at most what the partial buffer holds

An argument is `forced,sizing,epochs,CUs,format,small_window_ok,len,max_step,table / COUNTxL,shifts...` per channel group; format 0
plain, 2 high-dynamics, 3 complex chips, 4 16-bit."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

E1 = "/32x8184,-0.5,0,0.5"  # 32 channels of a Galileo E1 code, taps half a chip apart: spread 1.0, table 8184 + 64 = 8248
CA = "/8x1023,-0.5,0,0.5"  # 8 channels of a GPS C/A code: table 1087

# launch -> "n_slices lds_floats"
TABLE = [
    # 32 jobs on 256 CUs: ceil(2048 / 32) = 64; 196 chunks / 4 = 49.  Long plain code: max(49, ceil(8184 / 4096) = 2).  (100016 + 511) / 512 = 196
    # chunks, cps = 4: 2048 * 0.08184 * 1.002 + 1.0 = 168.94 -> 169 + 64 = 233 -> 256 -> the 1024 floor
    ("0,1,1,256,0,1,100000,0,8248" + E1, "49 1024"),
    # 8 x 64 = 512 jobs: ceil(2048 / 512) = 4; 8 chunks / 4 = 2.  len < 4096: the table stays whole
    ("0,1,64,256,0,1,4000,0,1087" + CA, "2 1087"),
    # 8 x 256 = 2048 jobs >= 2048: one slice; 2040 jobs: ceil(2048 / 2040) = 2
    ("0,1,256,256,0,1,4000,0,1087" + CA, "1 1087"),
    ("0,1,255,256,0,1,4000,0,1087" + CA, "2 1087"),
    # no CU count: 256, the two rows above again; 128 CUs: 2040 jobs >= 1024
    ("0,1,256,0,0,1,4000,0,1087" + CA, "1 1087"),
    ("0,1,255,0,0,1,4000,0,1087" + CA, "2 1087"),
    ("0,1,255,128,0,1,4000,0,1087" + CA, "1 1087"),
    # forced slices; a table within 4096 + 128 is left whole
    ("7,1,1,256,0,1,25000,0,1087/1x1023,-0.5,0,0.5", "7 1087"),
    # the 64 cap: one job, 391 chunks / 4 = 97
    ("0,1,1,256,0,1,200000,0,1087/1x1023,-0.5,0,0.5", "64 1087"),
    # sizing off: set_slices(-1), high-dynamics, 16-bit, a kernel without the small-window path; the slices stay those of the first row
    ("0,0,1,256,0,1,100000,0,8248" + E1, "49 8248"),
    ("0,1,1,256,2,1,100000,0,8248" + E1, "49 8248"),
    ("0,1,1,256,4,1,100000,0,8248" + E1, "49 8248"),
    ("0,1,1,256,0,0,100000,0,8248" + E1, "49 8248"),
    # len 4095: 8 chunks / 4 = 2, no sizing.  len 4096: max(2, ceil(8184 / 4096) = 2); (4096 + 16 + 511) / 512 = 9 chunks, cps = 5:
    # 2560 * 1.998046875 * 1.002 + 1.0 = 5126.23 -> 5127 + 64 = 5191 -> 5248
    ("0,1,1,256,0,1,4095,0,8248" + E1, "2 8248"),
    ("0,1,1,256,0,1,4096,0,8248" + E1, "2 5248"),
    # the long-code rule alone: 2048 jobs give 1 slice, a 10230-chip plain code ceil(10230 / 4096) = 3.  79 chunks, cps = 27:
    # 13824 * 0.25575 * 1.002 + 1.0 = 3543.56 -> 3544 + 64 = 3608 -> 3648
    ("0,1,2048,256,0,1,40000,0,10294/1x10230,-0.5,0,0.5", "3 3648"),
    # ... not when the slices are forced: cps = 40: 20480 * 0.25575 * 1.002 + 1.0 = 5249.24 -> 5250 + 64 = 5314 -> 5376
    ("2,1,1,256,0,1,40000,0,10294/1x10230,-0.5,0,0.5", "2 5376"),
    # ... and not for complex chips (5000 chips: table 2 * 5064 = 10128): one slice, nothing to size
    ("0,1,2048,256,3,1,40000,0,10128/1x5000,-0.5,0,0.5", "1 10128"),
    # complex chips double the need: 2 slices, cps = 40: 20480 * 0.125 * 1.002 + 1.0 = 2566.12 -> 2567 + 64 = 2631, twice: 5262 -> 5312;
    # the same code as plain chips (table 5064): 2631 -> 2688
    ("2,1,1,256,3,1,40000,0,10128/1x5000,-0.5,0,0.5", "2 5312"),
    ("2,1,1,256,0,1,40000,0,5064/1x5000,-0.5,0,0.5", "2 2688"),
    # one complex job: ceil(2048 / 1) = 2048, 79 chunks / 4 = 19; cps = 5: 2560 * 0.125 * 1.002 + 1.0 = 321.64 -> 322 + 64 = 386, twice: 772 -> 832 -> 1024
    ("0,1,1,256,3,1,40000,0,10128/1x5000,-0.5,0,0.5", "19 1024"),
    # the records' largest code step instead of l_max / len: 2048 * 1.0 * 1.002 + 1.0 = 2053.10 -> 2054 + 64 = 2118 -> 2176
    ("0,1,1,256,0,1,100000,1.0,8248" + E1, "49 2176"),
    # ... a step that needs more than the table: whole (2048 * 5.0 * 1.002 + 1.0 = 10261.48 -> 10262 + 64 = 10326 >= 8248)
    ("0,1,1,256,0,1,100000,5.0,8248" + E1, "49 8248"),
    # ... a huge step: 2048 * 1e9 * 1.002 = 2.05e12 is past what an int holds; the bound is compared as a double, the table stays whole
    ("0,1,1,256,0,1,100000,1e9,8248" + E1, "49 8248"),
    # the widest tap spread of any channel (100.25, the second one's) and the longest code of any (the first one's); 2 jobs: still 49 slices:
    # 2052.096 + 100.25 = 2152.35 -> 2153 + 64 = 2217 -> 2240
    ("0,1,1,256,0,1,100000,1.0,8248/1x8184,-0.5,0,0.5/1x1023,-50,0,50.25", "49 2240"),
    # a table of exactly 4096 + 128 floats is left whole, one float more is sized: 4 slices, 79 chunks, cps = 20:
    # 10240 * 0.104025 * 1.002 + 1.0 = 1068.35 -> 1069 + 64 = 1133 -> 1152
    ("4,1,1,256,0,1,40000,0,4224/1x4160,-0.5,0,0.5", "4 4224"),
    ("4,1,1,256,0,1,40000,0,4225/1x4161,-0.5,0,0.5", "4 1152"),
    # level 1: (N + 512) / 512 / 2
    ("l1:0,2048,64", "1"), ("l1:2048,2048,64", "1"), ("l1:2049,2048,64", "2"), ("l1:4000,2048,64", "4"), ("l1:4500,2048,64", "4"),
    ("l1:25000,2048,64", "24"), ("l1:100000,2048,64", "64"),  # 196 / 2 = 98: what the partial buffer holds
    ("l1:100000,2048,16", "16"), ("l1:4000,8192,64", "1"), ("l1:600,0,64", "1"),  # 2 chunks / 2; one chunk: never below 1
    ("l1:100,0,64", "1"),
]


def build(tmp_path_factory, flags):
    exe = str(tmp_path_factory.mktemp("trk_batch_plan") / "trk_batch_plan_selftest")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-Wall", "-Wextra"] + flags + ["-I", os.path.join(ROOT, "gnss-sdr-1_amd", "csrc"),
        os.path.join(ROOT, "tests", "trk_batch_plan_selftest.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan_ubsan"])
def test_plan_equals_the_hand_worked_table(tmp_path_factory, flags):
    exe = build(tmp_path_factory, flags)
    out = subprocess.run([exe] + [launch for launch, _ in TABLE], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == "", out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(TABLE)
    for (launch, want), line in zip(TABLE, got):
        assert line == want, "launch %s: plan %s, expected %s" % (launch, line, want)
