"""The host side of the launchers (falcon-r1cs_amd/csrc/frw_launch.h: the variant dispatcher, the residency table, resident_grid and
verify_shape) where no GPU is needed: the stand-alone program of tests/cpp/test_launch_host.cpp (its own main, nothing of it is loaded
into Python, nothing linked but the header), built with -fsanitize=address,undefined.  Every family's variant list is held to the set of
kernel instantiations, every tuple outside a list is refused without a call, index() is a bijection onto the table's slots, and the launch
shapes at 256 CUs are the ones computed before the arithmetic moved into the header (default FRW_OVERSUB, no FRW_FORCE_GRID)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpp", "test_launch_host.cpp")
INC = ["-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc")]


def test_dispatcher_tables_and_launch_shapes_are_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "launch_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror"] + INC + ["-o", exe, SRC])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert res.returncode == 0, res.stdout
    assert res.stdout.strip().endswith("launch_host: clean"), res.stdout
    assert "60 variants of 8 families dispatched, 44 launch shapes" in res.stdout
