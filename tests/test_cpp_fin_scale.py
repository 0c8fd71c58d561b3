"""The 32-bit plaintext scaling of the item kernel (csrc/hhe_fin_bodies.h: plain_fix32 / plain_scaled32, fin_item_store<T, true>, the
c1 slices of fin_item_c1; DESIGN.md "32-bit scaling"), driven from C++ (tests/cpp/fin_scale_main.cpp) as a stand-alone host program under
AddressSanitizer and UBSan: the new values equal plain_fix / plain_scaled and the definition floor((m Q + (t+1)/2) / t) mod q_j for every
m < 65537 and, at t = 1073479681, for the rounding-boundary coefficients and 10^6 random ones; the phases of the 32-bit instantiation looped
over 1024 threads write the words of the default instantiation and of add_plain_body, each exactly once; and the host's constants are
the quotients they are defined as."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scale32_matches_shared_definition_under_sanitizers(tmp_path):
    exe = tmp_path / "fin_scale"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",  # the runtimes are part of the program: it runs in any environment as it is
                           "-DHHE_RANGE_CHECK", "-I" + os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fin_scale_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "fin_scale OK" in r.stdout, r.stdout + r.stderr
