"""The decoder's parser of untrusted bytes (no GPU): image-webp_amd/csrc/
zw_dec_parse.cpp as an ordinary executable under the address and undefined-
behaviour sanitizers (tools/dec_parse_check.cpp).  Every golden stream parses
and the CPU replay of the device token parse writes the same records; prefixes
and byte flips of it fail with an error code or parse, never crash."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def test_parser_under_sanitizers(tmp_path):
    streams = sorted(glob.glob(os.path.join(GOLD, "*.vp8")))
    assert len(streams) >= 20
    exe = str(tmp_path / "dec_parse_check")
    csrc = os.path.join(ROOT, "image-webp_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", csrc, os.path.join(ROOT, "tools", "dec_parse_check.cpp"),
                           os.path.join(csrc, "zw_dec_parse.cpp"), "-o", exe])
    out = subprocess.run([exe] + streams, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    last = out.stdout.split()
    assert last[-3] == "ok" and int(last[-2]) == len(streams), out.stdout
    # 13 short prefixes, 24 spaced ones and 48 flipped copies of each stream
    assert int(last[-1]) == len(streams) * (13 + 24 + 48), out.stdout
