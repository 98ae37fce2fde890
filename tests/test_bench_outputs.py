"""not-gpu: bench.py's --dump-outputs sample and its argument checks, with a host stand-in for the device buffer."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


class _HostBuffer:
    """The part of fft_wgpu_amd.Buffer that dump_outputs uses, over a host array; refuses reads outside it as
    fwa_buf_download does."""

    def __init__(self, data):
        self.data = data
        self.reads = []

    def map_read(self, offset=0, size=None, stream=None, dtype=np.complex64):
        assert offset % 8 == 0 and size % 8 == 0 and offset + size <= self.data.nbytes
        self.reads.append((offset, size))
        return self.data[offset // 8:(offset + size) // 8].copy()


class _FW:
    COMPLEX_BYTES = 8


@pytest.mark.parametrize("n,batch,world", [(1 << 10, 64, 1), (1 << 10, 3, 1), (1 << 12, 512, 8), (1 << 23, 1, 1)])
def test_dump_is_a_seeded_sample_of_the_buffer_within_64_mb(tmp_path, n, batch, world):
    data = (np.arange(n * batch) + 1j * -np.arange(n * batch)).astype(np.complex64)
    buf = _HostBuffer(data)
    for rank in range(min(world, 2)):
        bench.dump_outputs(str(tmp_path), _FW, buf, None, n, batch, rank, world)
    names = sorted(os.listdir(tmp_path))
    assert names == (["spectrum.npy"] if world == 1 else ["spectrum_rank0.npy", "spectrum_rank1.npy"])
    got = np.load(tmp_path / names[0])
    assert got.dtype == np.float32 and got.ndim == 3 and got.shape[2] == 2
    assert got.nbytes * world <= 64 << 20 and got.shape[0] <= batch and got.shape[1] <= n
    first = [off // (8 * n) for off, _ in buf.reads[:got.shape[0]]]
    assert first == sorted(set(first))                    # distinct transforms, in order
    for i, t in enumerate(first):
        want = data[t * n:t * n + got.shape[1]]
        assert np.array_equal(got[i, :, 0], want.real) and np.array_equal(got[i, :, 1], want.imag)
    # the same arguments pick the same sample
    again = tmp_path / "again"
    bench.dump_outputs(str(again), _FW, _HostBuffer(data), None, n, batch, 0, world)
    assert np.array_equal(np.load(again / names[0]), got)


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--steps must be at least 1" in r.stderr
    assert '"n_gpus"' not in r.stdout
