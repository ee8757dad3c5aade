"""Host: the workgroup id -> tile maps of quadform_kernel (PPBO_QF_ORDER) and gram_mfma_kernel (PPBO_GRAM_VARIANT) are
bijections.  Both maps live in ppbo_amd/csrc/tile_walk.h as host/device functions that the kernels call;
tests/c/tile_walk_check.cpp runs the same functions on the host over every grid of 1..48 x 1..600 tiles and eleven orders
(contraction) and 1..160 tiles per side and both orders (Gram), under AddressSanitizer and UBSan.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_tile_is_walked_exactly_once(tmp_path):
    exe = tmp_path / "tile_walk_check"
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "c", "tile_walk_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "tile_walk_check ok" in r.stdout
