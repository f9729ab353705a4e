"""The host side of the bytes paths (falcon-r1cs_amd/csrc/frw_stage.h: circuit_shape, message_offsets_ok, StagedInputs) where no GPU is
needed: the stand-alone program of tests/cpp/test_stage_host.cpp (its own main, nothing of it is loaded into Python), built with
-fsanitize=address,undefined.  It stages batches of 5 and 7 in passes of 1, 2, 3 and 7 into heap buffers of exactly the reported size and
holds every piece to the plain slice of its source; and it holds circuit_shape to the counts of frw_layout*, which tests/test_capi.py and
tests/test_schoolbook_host.py hold to the reference's."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpp", "test_stage_host.cpp")
LIBDIR = os.path.join(ROOT, "falcon-r1cs_amd")
INC = ["-I", os.path.join(HERE, "cpp", "hip_host"), "-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc")]


def test_staging_and_circuit_shapes_are_clean_under_the_sanitizers(tmp_path):
    assert os.path.exists(os.path.join(LIBDIR, "libfrw.so")), "libfrw.so not built; run __graft_entry__.build()"
    exe = str(tmp_path / "stage_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror"] + INC + ["-o", exe, SRC, "-L" + LIBDIR, "-lfrw", "-Wl,-rpath," + LIBDIR])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")       # (the HIP runtime the library brings along keeps what it allocates at load)
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=120, env=env)
    assert res.returncode == 0, res.stdout
    assert res.stdout.strip().endswith("stage_host: clean"), res.stdout
    assert "32 batches staged pass by pass, 6 circuit shapes" in res.stdout
