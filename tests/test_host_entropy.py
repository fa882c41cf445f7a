"""Host entropy stage (no GPU): the batched boolean encoder of the serial
reference walk (tools/emit_ref.h) is byte-identical to the reference's
bit-at-a-time ArithmeticEncoder (encoder/arithmetic.rs:7-196) over random
decision streams (skewed and uniform probabilities, long carry runs); the
product's split emission (image-webp_amd/csrc/zw_host_emit.h: recorded
decisions, several frames' and partitions' coders side by side) is
byte-identical to that walk."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bool_encoder_batched_equals_reference(tmp_path):
    exe = str(tmp_path / "bool_equiv")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "image-webp_amd", "csrc"),
                           os.path.join(ROOT, "tools", "bool_equiv.cpp"), "-o", exe])
    out = subprocess.run([exe, "200000"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "equivalent" in out.stdout


def test_stats_token_paths_equal_reference_form(tmp_path):
    """record_coeffs via token paths == the reference's branchy record_coeffs
    (cost.rs:1297, never-cleared skip_eob), accumulated so the 0xfffe0000
    halving is exercised."""
    exe = str(tmp_path / "stats_equiv")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "image-webp_amd", "csrc"),
                           os.path.join(ROOT, "tools", "stats_equiv.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "equivalent" in out.stdout, out.stdout + out.stderr


def _emit_equiv(tmp_path, flags):
    exe = str(tmp_path / "emit_equiv")
    subprocess.check_call(["g++", "-std=c++17", *flags, "-I", os.path.join(ROOT, "image-webp_amd", "csrc"),
                           os.path.join(ROOT, "tools", "emit_equiv.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "equivalent" in out.stdout, out.stdout + out.stderr
    return out.stdout


def test_split_emission_equals_frame_walk(tmp_path):
    """zwh::emit_frames (K frames x 1, 2, 4, 8 token partitions, up to 16
    streams: decisions recorded per MB row, the streams' coders side by side)
    == the serial walk zwh::emit_frame (tools/emit_ref.h) on random packed
    records (every luma mode, skips, segments, sub-modes, all token categories,
    frame headers with and without probability updates, fewer MB rows than
    partitions and row counts they do not divide), and the interleaved and
    16-lane coders == the bit-at-a-time reference over random streams coded in
    pieces.  Then a workspace whose token arena failed to grow (operator new[]
    made to throw once) emits the reference's bytes again."""
    out = _emit_equiv(tmp_path, ["-O2"])
    assert "failed growth survived" in out, out


def test_split_emission_under_sanitizers(tmp_path):
    """The same program as an ordinary executable under the address and
    undefined-behaviour sanitizers (without the failed-growth part: it
    replaces operator new[])."""
    out = _emit_equiv(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "failed growth" not in out, out
