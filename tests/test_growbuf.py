"""GrowBuf<T>, the one grow-only device workspace type of the host driver (csrc/hhe_internal.h), driven from C++
(tests/cpp/growbuf_main.cpp) against logging stubs of rt_malloc / rt_free / sync_ctx whose allocator can be told to fail: a request
within the capacity makes no call; growth waits exactly once, before the free; a failed growth leaves {null, 0} and HHE_ERR_DEVICE,
and the next request of a size that used to fit allocates again; release() frees once and may be repeated."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_growbuf_contract(tmp_path):
    exe = tmp_path / "growbuf"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "privacy-preserving-ml-through-hhe_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "growbuf_main.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "growbuf OK" in r.stdout, r.stdout + r.stderr
