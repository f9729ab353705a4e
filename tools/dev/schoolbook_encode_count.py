"""Instruction counts of the two probe kernels of tools/dev/schoolbook_encode_probe.hip from the emitted gfx950 assembly (no GPU):
python tools/dev/schoolbook_encode_count.py   ->  one line per kernel: all instructions, vector ALU, 64-bit multiply-adds, memory."""
import os
import re
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "probe.s")
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-w", "--cuda-device-only", "-S",
                               os.path.join(HERE, "schoolbook_encode_probe.hip"), "-o", asm])
        text = open(asm).read()
    for name in ("probe_cios", "probe_small"):
        m = re.search(r"^_ZN3frw\d+%s\w*:[^\n]*\n(.*?)s_endpgm" % name, text, re.S | re.M)
        ops = [ln.split()[0] for ln in m.group(1).splitlines() if re.match(r"\s+[sv]_|\s+(global|buffer|ds|flat)_", ln)]
        valu = [o for o in ops if o.startswith("v_")]
        print("%-12s instructions %4d  vector ALU %4d  v_mad_u64_u32 %3d  v_mul_* %3d  memory %3d" % (
            name, len(ops), len(valu), valu.count("v_mad_u64_u32"), sum(o.startswith("v_mul_") for o in valu),
            sum(o.startswith(("global_", "buffer_", "flat_")) for o in ops)))


if __name__ == "__main__":
    main()
