"""The way in for a constraint system that comes as matrices (falcon-r1cs_amd/csrc/frw_r1cs_file.h; frw_r1cs_load_csr and
frw_r1cs_load_file of include/frw.h) where no GPU is needed: the stand-alone program of tests/cpp/test_r1cs_file_host.cpp (its own main,
nothing of it is loaded into Python), built with -fsanitize=address,undefined.  The Falcon-512 export parsed and written again gives the
same bytes; every refusal frw.h lists is refused with the matrix and the row named, files one byte short and one byte long too; a repeated
column, a zero coefficient, an empty row and an unused variable are accepted; and through the library a malformed system is
FRW_E_INVALID_ARG and a well-formed one FRW_E_NO_DEVICE -- on device -1, which no machine has, so validation is seen to come first
whether or not there is a GPU."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpp", "test_r1cs_file_host.cpp")
LIBDIR = os.path.join(ROOT, "falcon-r1cs_amd")
INC = ["-I", os.path.join(ROOT, "falcon-r1cs_amd", "csrc")]


def test_parsing_and_validation_are_clean_under_the_sanitizers(tmp_path):
    assert os.path.exists(os.path.join(LIBDIR, "libfrw.so")), "libfrw.so not built; run __graft_entry__.build()"
    exe = str(tmp_path / "r1cs_file_host_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-Werror"] + INC + ["-o", exe, SRC, "-L" + LIBDIR, "-lfrw", "-Wl,-rpath," + LIBDIR])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")       # (the HIP runtime the library brings along keeps what it allocates at load)
    work = tmp_path / "files"
    work.mkdir()
    res = subprocess.run([exe, str(work)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout
    assert res.stdout.strip().endswith("r1cs_file_host: clean"), res.stdout
    assert "37 cases" in res.stdout, res.stdout
