"""KsCache, the bookkeeping of the keystream ciphertexts kept across transciphering calls (csrc/hhe_kscache.h), driven from C++
(tests/cpp/kscache_main.cpp) against logging stubs of rt_malloc / rt_free / sync_ctx, as a stand-alone host program under
AddressSanitizer and UBSan: insert, hit, evict by budget, evict by block table, key-set destroy, snapshot turnover, clear, context
destroy -- every buffer freed exactly once, behind one wait, and no entry reachable after its owner went."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kscache_bookkeeping_under_sanitizers(tmp_path):
    exe = tmp_path / "kscache"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",  # the runtimes are part of the program: it runs in any environment as it is
                           "-I" + os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "kscache_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "kscache OK" in r.stdout, r.stdout + r.stderr
