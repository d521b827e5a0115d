"""Constructor unwinding of the model executors, outside Python: tests/native/unwind_main.cpp is compiled alone with the host
AddressSanitizer, linked against the built library and run as an ordinary executable with nothing preloaded.  Every model class
must throw maa::Error on an empty state dict, and LeakSanitizer's report at exit may attribute no leak to a maa:: frame (at the
commit before the executors held their Impl in a unique_ptr it names UNet, VAE, Vocoder and DiffNet)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constructors_that_throw_leak_nothing(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a host-sanitizer build is run on machines without a GPU only")
    from audiogpt_amd import build
    lib = build.build(verbose=False)
    exe = str(tmp_path / "unwind_main")
    san = ["-Xarch_host", "-fsanitize=address", "-Xarch_host", "-fno-omit-frame-pointer"]
    cmd = [build._hipcc(), "--offload-arch=" + build.ARCH, "-std=c++17", "-x", "hip", "-g"] + san + \
        [os.path.join(ROOT, "tests", "native", "unwind_main.cpp"), "-o", exe, "-fsanitize=address",
         "-L" + os.path.dirname(lib), "-laudiogpt_mi355x", "-Wl,-rpath," + os.path.dirname(lib)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if k not in ("LD_PRELOAD", "ASAN_OPTIONS", "LSAN_OPTIONS")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert "UNWIND_OK" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.count("ok   ") == 24, r.stdout
    assert "maa::" not in r.stderr, r.stderr[-8000:]
    assert r.returncode == 0, r.stderr[-8000:]
