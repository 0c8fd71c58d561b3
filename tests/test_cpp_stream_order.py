"""The stream model of the tests-only emulator (tests/emu/emu_order.cpp) pinned on its own, as a stand-alone host program
(tests/cpp/stream_order_main.cpp) under AddressSanitizer and UBSan.  Nothing of the library's host driver is in it: two trivial
operations on the rt_* layer show each rule of the lazy order in both directions -- a consumer without an event reads the poison, one
behind record + wait reads the data; a wait binds to the record enqueued before it; a force runs the minimum; page-locked and pageable
host memory; free forces everything -- and that the eager order runs everything inside the call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_model_rules_under_sanitizers(tmp_path):
    exe = tmp_path / "stream_order"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",  # the runtimes are part of the program: it runs in any environment as it is
                           "-I" + os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"), "-I" + os.path.join(ROOT, "tests", "emu"),
                           os.path.join(ROOT, "tests", "cpp", "stream_order_main.cpp"), os.path.join(ROOT, "tests", "emu", "emu_order.cpp"),
                           "-o", str(exe)])
    env = {k: v for k, v in os.environ.items() if k != "HHE_EMU_ORDER"}
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "stream_order OK" in r.stdout, r.stdout + r.stderr
