"""The finishing pass with one workgroup per item (csrc/hhe_fin_bodies.h: encode into LDS, the whole inverse transform mod t in 32-bit
words, add_plain epilogue), driven from C++ (tests/cpp/fin_item_main.cpp) as a stand-alone host program under AddressSanitizer and
UBSan: its phases looped over 1024 threads must write the words of the launches it replaces (encode_scatter_body, an inverse transform evaluated
directly, add_plain_body), at N = 2^10, 2^12 and 2^14, for counts 0 / 1 / 127 / 128, words that are not reduced, and keystreams given by table and by
stride."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_item_body_matches_separate_launches_under_sanitizers(tmp_path):
    exe = tmp_path / "fin_item"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",  # the runtimes are part of the program: it runs in any environment as it is
                           "-DHHE_RANGE_CHECK", "-I" + os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fin_item_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "fin_item OK" in r.stdout, r.stdout + r.stderr
