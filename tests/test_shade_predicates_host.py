"""pt_device.h's range predicates on the CPU: shade_lane's coord_ok_m, dir_ok_m and ray_fast_m are mask arithmetic
('&' / '|' on int); their host twins -- the same functions, compiled for the host -- must have the truth tables of
the '&&' / '||' forms coord_ok, dir_ok and ray_fast, over the edge grid 0, +-2^-101, +-2^-100, +-2^-51, +-2^-50, +-2^20 and the float above,
+-2^45 and the float above, inf and NaN (tests/shade_pred_probe.cpp)."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_mask_predicates_equal_the_short_circuit_forms(tmp_path):
    exe = str(tmp_path / "shade_pred_probe")
    csrc = os.path.join(ROOT, "cudapathtracer_amd", "csrc")
    subprocess.check_call([HIPCC, "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-x", "hip",
                           "--offload-arch=gfx950", "--cuda-host-only", "-I" + os.path.join(csrc, "hip"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "shade_pred_probe.cpp"),
                           "-o", exe], timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith(": 0 mismatches")
