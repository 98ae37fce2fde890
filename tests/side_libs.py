"""Build, import and load one side plan library -- strided, fft2d, real, conv or stft (TEST INFRASTRUCTURE ONLY): what the
fixtures of tests/test_<lib>.py and tests/test_gpu_<lib>.py share.  The library is built by the session that needs it
(tests/conftest.py builds csrc only); its Makefile builds what it links against first."""
import importlib
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("strided", "fft2d", "real", "conv", "stft")  # build order: fft2d links against strided


def directory(name):
    return os.path.join(ROOT, "fft_wgpu_amd", name)


def load(name):
    """make -C fft_wgpu_amd/<name>, then fft_wgpu_amd.<name> with its library loaded."""
    assert name in NAMES, name
    subprocess.check_call(["make", "-s", "-C", directory(name)])
    m = importlib.import_module("fft_wgpu_amd." + name)
    m.lib()
    return m
