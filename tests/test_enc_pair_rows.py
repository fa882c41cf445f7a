"""Pass 1's frame-pair row schedule (no GPU): PairRowSchedule1 in
image-webp_amd/csrc/zw_enc_rows.h walked on the host for every frame height
from 1 to 300 MB rows (tools/enc_pair_rows_check.cpp) -- one owner per row,
every wave's rows strictly increasing, no chain wave above the join row, no
join under the floor, the walk run to its end as the kernel runs it, and the
shipped order at 68 rows pinned.  On the device a wrong schedule is a hang."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "image-webp_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "enc_pair_rows_check.cpp")


def _run(tmp_path, name, defs=()):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O2", "-std=c++17", *defs, "-I", CSRC, TOOL, "-o", exe])
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_pair_row_schedule(tmp_path):
    out = _run(tmp_path, "enc_pair_rows_check")
    assert out.returncode == 0 and "ok" in out.stdout and "not pinned" not in out.stdout, out.stdout + out.stderr


def test_pair_row_schedule_other_knobs(tmp_path):
    """The checks hold for the knobs' other settings too (those measured and
    the corners: no slow rows, no join, a join at row 0)."""
    for i, defs in enumerate((("-DZW_P1P_SLOW_NUM=2", "-DZW_P1P_JOIN_NUM=1", "-DZW_P1P_JOIN_DEN=2"),
                              ("-DZW_P1P_SLOW_NUM=3", "-DZW_P1P_SLOW_DEN=2"),
                              ("-DZW_P1P_SLOW_NUM=0", "-DZW_P1P_JOIN_MIN=1"),
                              ("-DZW_P1P_JOIN_NUM=1", "-DZW_P1P_JOIN_DEN=1"),
                              ("-DZW_P1P_JOIN_NUM=0", "-DZW_P1P_JOIN_MIN=13"))):
        out = _run(tmp_path, "enc_pair_rows_check_%d" % i, defs)
        assert out.returncode == 0 and "ok" in out.stdout, (defs, out.stdout + out.stderr)
