"""The resample form a phd_step takes (csrc/phd_step_plan.h), without a GPU:
tests/step_plan_harness.cpp is built with a host compiler and asked for a table
of facts.  The expected forms are written out from the rules the step follows
(DESIGN.md §4.3), each boundary from both sides."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NONE, BLOCK, STEP, CHUNKS, BESIDE, LEAD, SEPARATE = range(7)  # PHD_RS_FORM_* (include/phd_capi.h)
PHD, CPHD = 0, 1
STATIC, MIXED = 0, 2

FIELDS = ["n", "n_base", "npp", "M", "filter", "feature", "split", "resident", "lds", "rs_lds", "traced", "stamps",
          "overlap", "lead"]


def rs_step_lds(nt):
    """rs_step_lds of phd_kernels.h: four [16][16] tables of 8-byte words, 16
    chunk ends, nt/64 + 1 floats, two ints."""
    return 4 * 16 * 16 * 8 + 16 * 8 + (nt // 64 + 1) * 4 + 2 * 4


# a CPHD step of 4096 particles whose part C is 2.7 rounds of 1536 resident
# workgroups with room for the lead workgroup's tables: the shipped lead form
BASE = dict(n=4096, n_base=4096, npp=1, M=10, filter=CPHD, feature=STATIC, split=1, resident=1536, lds=27000,
            rs_lds=rs_step_lds(256), traced=0, stamps=0, overlap=3, lead=1)
PHD_FUSED = dict(filter=PHD, split=0)
PHD_SPLIT = dict(filter=PHD, split=1)

# (what differs from BASE, form, fuse_max)
TABLE = [
    (dict(), LEAD, 1),
    # one block up to 2048 entries, chunked above
    (dict(n=2048, n_base=2048), BLOCK, 1),
    (dict(n=2049, n_base=2049), LEAD, 1),
    (dict(n=2048, n_base=2048, **PHD_FUSED), BLOCK, 1),
    (dict(n=2049, n_base=2049, **PHD_FUSED), STEP, 1),
    (dict(n=2048, n_base=2048, M=0), BLOCK, 1),
    # the chunked form fuses its max up to 16 chunks; four launches above (and nothing beside part C)
    (dict(n=16384, n_base=16384, **PHD_FUSED), STEP, 1),
    (dict(n=16385, n_base=16385, **PHD_FUSED), CHUNKS, 0),
    (dict(n=16384, n_base=16384, resident=4096), LEAD, 1),
    (dict(n=16385, n_base=16385, resident=8192), CHUNKS, 0),
    # beside / in front of part C only up to four rounds of its resident workgroups
    (dict(n=6144, n_base=6144), LEAD, 1),
    (dict(n=6145, n_base=6145), STEP, 1),
    (dict(n=6144, n_base=6144, lead=0), BESIDE, 1),
    (dict(n=6145, n_base=6145, lead=0), STEP, 1),
    # the lead workgroup needs its tables in part C's LDS
    (dict(lds=rs_step_lds(256) - 1), BESIDE, 1),
    (dict(lds=rs_step_lds(256)), LEAD, 1),
    (dict(lds=rs_step_lds(512) - 1, rs_lds=rs_step_lds(512)), BESIDE, 1),
    (dict(lds=rs_step_lds(512), rs_lds=rs_step_lds(512)), LEAD, 1),
    (dict(lds=rs_step_lds(1024) - 1, rs_lds=rs_step_lds(1024)), BESIDE, 1),
    (dict(lds=rs_step_lds(1024), rs_lds=rs_step_lds(1024)), LEAD, 1),
    # a traced step, an empty scan, the mixed model: after the update, on the context stream
    (dict(traced=1), STEP, 1),
    (dict(traced=1, lead=0), STEP, 1),
    (dict(M=0), STEP, 1),
    (dict(feature=MIXED), STEP, 1),
    # the diagnostic stamps build keeps the second stream
    (dict(stamps=1), BESIDE, 1),
    # PHD: only the split update has a part C
    (dict(**PHD_FUSED), STEP, 1),
    (dict(**PHD_SPLIT), LEAD, 1),
    (dict(lead=0, **PHD_SPLIT), BESIDE, 1),
    # live count above n_particles, or growing with this step's predict: the separate kernels
    (dict(n=8192), SEPARATE, 1),
    (dict(n=1000, n_base=500), SEPARATE, 1),
    (dict(n=20000, n_base=4096), SEPARATE, 0),
    (dict(npp=2), SEPARATE, 1),
    (dict(npp=2, n=1024, n_base=1024), SEPARATE, 1),
    # PHD_RS_LEAD 0: the second stream
    (dict(lead=0), BESIDE, 1),
    # PHD_RS_OVERLAP: bit 1 the CPHD step, bit 2 the split PHD step
    (dict(overlap=0), STEP, 1),
    (dict(overlap=0, **PHD_SPLIT), STEP, 1),
    (dict(overlap=1), LEAD, 1),
    (dict(overlap=1, **PHD_SPLIT), STEP, 1),
    (dict(overlap=2), STEP, 1),
    (dict(overlap=2, **PHD_SPLIT), LEAD, 1),
    (dict(overlap=3), LEAD, 1),
    (dict(overlap=3, **PHD_SPLIT), LEAD, 1),
    (dict(overlap=3, **PHD_FUSED), STEP, 1),
]


def test_rs_step_lds_formula():
    assert [rs_step_lds(nt) for nt in (256, 512, 1024)] == [8348, 8364, 8396]


def test_step_plan_table(tmp_path):
    cxx = next((c for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"),
                            "/opt/rocm/lib/llvm/bin/clang++") if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler present")
    exe = str(tmp_path / "step_plan_harness")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-I" + os.path.join(REPO, "include"), "-I" + os.path.join(REPO, "cuda-phdslam_amd", "csrc"),
                        os.path.join(REPO, "tests", "step_plan_harness.cpp"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    rows = [dict(BASE, **d) for d, _, _ in TABLE]
    text = "".join(" ".join(str(row[k]) for k in FIELDS) + "\n" for row in rows)
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(TABLE)
    wrong = [(d, g, (form, fuse)) for (d, form, fuse), g in zip(TABLE, got) if g != (form, fuse)]
    assert not wrong, wrong
