"""not-gpu: the C-ABI library loads, exports every symbol include/fft_wgpu_amd.h declares, and fails
loudly (status codes, no fallback) when there is no device."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def _header_functions():
    text = open(os.path.join(ROOT, "include", "fft_wgpu_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(fwa_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from fft_wgpu_amd import _ffi
    L = _ffi.lib()
    names = _header_functions()
    assert len(names) >= 28
    for name in names:
        assert hasattr(L, name), f"{name} declared in the header but not exported"
    # and the ctypes table covers the header exactly
    assert sorted(_ffi._SIGNATURES) == names
    assert L.fwa_abi_version() == 4


def test_laboratory_library_has_the_same_abi_and_the_product_has_no_laboratory_kernels():
    """the slower kernel families live in libfft_wgpu_amd_lab.so only.  Same exported ABI; the
    product library's device code contains none of the laboratory kernels."""
    import subprocess
    from fft_wgpu_amd import _ffi
    lab = _ffi.lib(lab=True)
    for name in _header_functions():
        assert hasattr(lab, name), f"{name} missing from the laboratory library"
    assert lab.fwa_abi_version() == _ffi.lib().fwa_abi_version()
    lab_kernels = (b"k_ring_1m", b"k_small16")
    prod = open(_ffi.LIB_PATH, "rb").read()
    labb = open(_ffi.LAB_LIB_PATH, "rb").read()
    for k in lab_kernels:
        assert k not in prod, f"{k!r} found in the product library"
        assert k in labb, f"{k!r} missing from the laboratory library"
    # families removed in round 6 (profiles/round6/lab_pruned_families.patch) are in neither library
    for k in (b"k_team", b"k_lds_small", b"k_tiny16", b"k_tiny2", b"k_p1_1mILin1ELi32E", b"k_p1_genILin1ELi2E"):
        assert k not in prod and k not in labb, k
    assert b"k_p1_1mILin1EE" in prod and b"k_colsw" in prod and b"k_rows32" in prod
    # only tools/ and the laboratory tests ask for the laboratory build
    hits = subprocess.run(["grep", "-rlE", r"lab=True|lab=args\.lab|LAB_LIB_PATH", "--include=*.py", ROOT],
                          capture_output=True, text=True).stdout.split()
    rel = sorted(os.path.relpath(h, ROOT) for h in hits)
    assert all(r.startswith(("tools/", "tests/")) or r in ("fft_wgpu_amd/_ffi.py", "fft_wgpu_amd/device.py") for r in rel), rel
    assert not any(r in ("bench.py", "__graft_entry__.py") for r in rel)


def test_rust_shim_declares_exactly_the_header_symbols():
    """rust_shim/ cannot be compiled here (no rustc): at least its `extern "C"` block must name exactly the functions
    include/fft_wgpu_amd.h declares, and its plans must keep the reference's public signatures."""
    ffi = open(os.path.join(ROOT, "rust_shim", "src", "ffi.rs")).read()
    rust_names = sorted(set(re.findall(r"pub fn (fwa_[a-z0-9_]+)\(", ffi)))
    assert rust_names == _header_functions()
    proc = open(os.path.join(ROOT, "rust_shim", "src", "processor.rs")).read()
    flat = re.sub(r"\s+", " ", proc)
    for plan in ("Forward", "Inverse"):
        assert f"impl<'a> {plan}<'a> {{ pub fn new(device: &'a wgpu::Device, queue: &'a wgpu::Queue, src: &'a wgpu::Buffer, fft_len: u32) -> Self" in flat
    assert ("impl<'a> Onlyinverse<'a> { pub fn new( device: &'a wgpu::Device, queue: &'a wgpu::Queue, src: &'a wgpu::Buffer, "
            "src2: &'a wgpu::Buffer, fft_len: u32, ) -> Self") in flat
    assert ("impl<'a> Normalize<'a> { pub fn new( device: &'a wgpu::Device, queue: &'a wgpu::Queue, buffer1: &'a wgpu::Buffer, "
            "buffer2: &'a wgpu::Buffer, fft_len: u32, ) -> Self") in flat
    assert flat.count("pub fn proc(&self, encoder: &mut wgpu::CommandEncoder) -> &wgpu::Buffer") == 4
    lib = open(os.path.join(ROOT, "rust_shim", "src", "lib.rs")).read()
    assert "pub struct Complex" in lib and "pub real: f32" in lib and "pub imag: f32" in lib and "pub mod wgpu_helper;" in lib


def test_rust_shim_is_sound_and_covers_the_wgpu_surface_of_the_reference_examples():
    """VERDICT round 2, item 6 (the crate is still uncompiled source: no rustc).  (1) No plan writes through a shared
    reference: the result-buffer handle sits in a Cell.  (2) Every `wgpu::` path and every wgpu method the reference's
    three examples use (src/examples/basic.rs:6-30,50-64,68,73-122; the same lines of basic_inverse.rs, basic_inverse2.rs --
    the list below was read off those files) is defined by rust_shim/src/wgpu_helper.rs, and rust_shim/examples/basic.rs
    exercises each of them."""
    src = {n: open(os.path.join(ROOT, "rust_shim", "src", n)).read() for n in ("processor.rs", "wgpu_helper.rs", "lib.rs")}
    proc = src["processor.rs"]
    assert "as *mut wgpu::Buffer" not in proc and "as *const wgpu::Buffer" not in proc and "(*slot)" not in proc
    assert proc.count("self.buffer_b.h.set(res)") == 2                      # Forward::proc, Inverse::proc
    helper = src["wgpu_helper.rs"]
    assert "pub(crate) h: Cell<*mut fwa_buf>" in helper
    paths = ["Instance::default", "RequestAdapterOptions", "PowerPreference::HighPerformance", "DeviceDescriptor", "BufferDescriptor",
             "BufferUsages::COPY_DST", "BufferUsages::COPY_SRC", "BufferUsages::MAP_READ", "BufferUsages::STORAGE",
             "CommandEncoderDescriptor", "Maintain::wait", "MapMode::Read"]
    defs = {"Instance::default": "#[derive(Default)]\npub struct Instance;", "RequestAdapterOptions": "pub struct RequestAdapterOptions",
            "PowerPreference::HighPerformance": "HighPerformance,", "DeviceDescriptor": "pub struct DeviceDescriptor<'a>",
            "BufferDescriptor": "pub struct BufferDescriptor<'a>", "BufferUsages::COPY_DST": "pub const COPY_DST: BufferUsages",
            "BufferUsages::COPY_SRC": "pub const COPY_SRC: BufferUsages", "BufferUsages::MAP_READ": "pub const MAP_READ: BufferUsages",
            "BufferUsages::STORAGE": "pub const STORAGE: BufferUsages", "CommandEncoderDescriptor": "pub struct CommandEncoderDescriptor<'a>",
            "Maintain::wait": "pub fn wait() -> Self", "MapMode::Read": "pub enum MapMode {\n    Read,"}
    for p in paths:
        assert defs[p] in helper, p
    methods = ["pub fn request_adapter(&self", "pub fn request_device(", "pub fn features(&self)", "pub fn limits(&self)",
               "pub fn create_buffer(&self", "pub fn slice<R: RangeBounds<u64>>(&self", "pub fn map_async(&self", "pub fn get_mapped_range(&self)",
               "pub fn unmap(&self)", "pub fn poll(&self, _maintain: Maintain) -> MaintainResult", "pub fn panic_on_timeout(self)",
               "pub fn create_command_encoder(&self", "pub fn copy_buffer_to_buffer(&mut self", "pub fn finish(self) -> CommandBuffer",
               "pub fn submit<I: IntoIterator<Item = CommandBuffer>>(&self", "pub fn write_buffer(&self", "impl BitOr for BufferUsages",
               "impl Deref for BufferView", "-> Ready<Option<Adapter>>", "-> Ready<Result<(Device, Queue), RequestDeviceError>>"]
    for m in methods:
        assert m in helper, m
    example = open(os.path.join(ROOT, "rust_shim", "examples", "basic.rs")).read()
    for p in paths:
        assert "wgpu::" + p in example, p
    for call in (".request_adapter(", ".request_device(", ".await", ".slice(..)", ".map_async(", ".panic_on_timeout()", ".get_mapped_range()",
                 ".unmap()", ".copy_buffer_to_buffer(", "queue.submit(Some(encoder.finish()))", "queue.write_buffer("):
        assert call in example, call
    assert "pub use wgpu_helper as wgpu;" in src["lib.rs"]
    # the reference lists its adapters (src/lib.rs:33-35: instance.enumerate_adapters(Backends::VULKAN));
    # the stand-in has the same call, one adapter per usable ordinal of fwa_device_count, and prepare_gpu goes through it
    for item in ("pub fn enumerate_adapters(&self, backends: Backends) -> Vec<Adapter>", "pub struct Backends(pub u32);",
                 "pub const VULKAN: Backends", "pub const GL: Backends", "pub const METAL: Backends", "pub fn get_info(&self) -> AdapterInfo",
                 "fwa_device_info(ordinal,", "fwa_device_count(&mut n)"):
        assert item in helper, item
    assert "instance.enumerate_adapters(wgpu::Backends::all())" in src["lib.rs"] and "pub mod sharded;" in src["lib.rs"]
    sharded = open(os.path.join(ROOT, "rust_shim", "src", "sharded.rs")).read()
    for item in ("pub fn slab(batch: u64, rank: i32, world: i32) -> (u64, u64)", "fwa_slab(batch, rank, world,", "pub fn open_shards(",
                 "instance.enumerate_adapters(wgpu::Backends::all())", "pub struct ShardedBatch<'a, P: ShardPlan<'a>>", "fwa_comm_scatter(", "fwa_comm_gather("):
        assert item in sharded, item


def test_no_device_is_an_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    import fft_wgpu_amd as fw
    assert fw.prepare_gpu(0) is None                      # lib.rs:29,43: Option -> None
    with pytest.raises(fw.FwaError) as e:
        fw.Device(0)
    assert e.value.status == 5                            # FWA_ERR_NO_DEVICE
    assert "device" in e.value.detail.lower()


def test_null_handles_are_rejected():
    from fft_wgpu_amd import _ffi
    L = _ffi.lib()
    out = ctypes.c_void_p()
    assert L.fwa_plan_create(None, 0, 1024, None, None, ctypes.byref(out)) == 1
    assert L.fwa_plan_exec(None, None, None) == 1
    assert L.fwa_buf_alloc(None, 16, ctypes.byref(out)) == 1
    assert L.fwa_stream_synchronize(None) == 1
    assert L.fwa_buf_free(None) == 0 and L.fwa_plan_destroy(None) == 0
    assert L.fwa_status_string(5) == b"no usable device"


def test_product_path_does_not_touch_the_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "fft_wgpu_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text and "ref_fft" not in text.replace(
                    "oracle/ref_fft.c", ""), f


def test_cpp_mirror_compiles_against_the_header(tmp_path):
    """include/fft_wgpu.hpp (the C++ host mirror) and the C++ replay of examples/basic_inverse2.rs build
    against the C ABI; without a GPU the binary must fail with FWA_ERR_NO_DEVICE, not fall back."""
    import subprocess
    import torch
    exe = tmp_path / "example"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tools", "example_basic_inverse2.cpp"),
                           "-L" + os.path.join(ROOT, "fft_wgpu_amd"), "-lfft_wgpu_amd", "-pthread", "-o", str(exe)])
    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(ROOT, "fft_wgpu_amd") + ":" + os.environ.get("LD_LIBRARY_PATH", ""))
    r = subprocess.run([str(exe)], env=env, capture_output=True, text=True)
    if torch.cuda.is_available():
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode == 2 and "error 5" in r.stderr


def test_path_selection_host_logic():
    """fwa_describe_path: the plan's path/factorisation logic runs without a device."""
    import fft_wgpu_amd as fw
    assert fw.describe_path(1) == (4, [])                       # identity
    for lg in range(1, 16):
        assert fw.describe_path(1 << lg) == (0, [1 << lg])      # one-launch kernels up to 32768
    assert fw.describe_path(1 << 20) == (1, [1024, 1024])       # headline two-pass pipeline
    assert fw.describe_path(1 << 24) == (7, [512, 128, 256])    # config C5: 512 x 32-column first pass (k_colsw)
    assert fw.describe_path(1 << 16) == (7, [256, 256])         # 256 x 64-column first pass (k_colsw)
    assert fw.describe_path(1 << 19) == (7, [512, 1024])
    assert fw.describe_path(1 << 22) == (7, [1024, 4096])       # two passes: k_p1_gen + k_rows32 (4096-point rows)
    assert fw.describe_path(1 << 23) == (7, [2048, 4096])       # two passes: k_cols32 + k_rows32
    assert fw.describe_path(1 << 30) == (7, [1024, 1024, 1024])
    assert fw.describe_path(1 << 21) == (7, [1024, 2048])       # two passes: 2048-point rows in k_rows32
    for lg in list(range(16, 20)) + list(range(21, 31)):
        path, f = fw.describe_path(1 << lg)
        assert path == 7 and all(64 <= x <= (4096 if lg in (21, 22, 23) else 1024) for x in f)
        prod = 1
        for x in f:
            prod *= x
        assert prod == 1 << lg and len(f) == (2 if lg <= 19 or lg in (21, 22, 23) else 3)
    with pytest.raises(fw.FwaError) as e:
        fw.describe_path(1000)
    assert e.value.status == 1
    with pytest.raises(fw.FwaError):
        fw.describe_path(0)


def test_header_is_plain_c(tmp_path):
    """The boundary must be consumable from C (and hence from Rust bindgen / cgo / JNI): C99, no warnings."""
    import subprocess
    src = tmp_path / "c_user.c"
    src.write_text('#include "fft_wgpu_amd.h"\n'
                   'int probe(void) { fwa_ctx *c = 0; int32_t n = 0; (void)c; return fwa_device_count(&n) + fwa_abi_version(); }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "c_user.o")])


def _stub_library(tmp_path, version, name="libfft_wgpu_amd.so"):
    """A shared library that only answers fwa_abi_version (what a stale build beside newer host code looks like)."""
    import subprocess
    src = tmp_path / "stub.c"
    src.write_text("#include <stdint.h>\nint32_t fwa_abi_version(void) { return %d; }\n" % version)
    out = tmp_path / name
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", str(out)])
    return out


def test_python_mirror_refuses_a_library_of_another_abi_version(tmp_path):
    """`_ffi.lib()` compares fwa_abi_version() with the version the binding was written for when it
    LOADS the library -- a stale .so reporting version 3 is refused before any signature is bound or any entry point called."""
    import re
    from fft_wgpu_amd import _ffi
    header = open(os.path.join(ROOT, "include", "fft_wgpu_amd.h")).read()
    assert _ffi.ABI_VERSION == int(re.search(r"#define FWA_ABI_VERSION (\d+)", header).group(1))
    stub = _stub_library(tmp_path, _ffi.ABI_VERSION - 1)
    with pytest.raises(RuntimeError) as e:
        _ffi.lib(str(stub))
    assert f"ABI version {_ffi.ABI_VERSION - 1}" in str(e.value) and "rebuild" in str(e.value)
    assert str(stub) not in _ffi._libs                      # a refused library is not cached as loaded
    nothing = tmp_path / "libempty.so"                       # a library without the symbol at all is refused the same way
    import subprocess
    (tmp_path / "empty.c").write_text("int unrelated;\n")
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(tmp_path / "empty.c"), "-o", str(nothing)])
    with pytest.raises(RuntimeError) as e:
        _ffi.lib(str(nothing))
    assert "ABI version None" in str(e.value)


def test_cpp_mirror_refuses_a_library_of_another_abi_version(tmp_path):
    """fft_wgpu::Device's constructor (and enumerate_devices) throw Error(FWA_ERR_UNSUPPORTED) when the library found at run
    time reports another FWA_ABI_VERSION than the header the host was compiled against -- before fwa_ctx_create is reached
    (the stub does not even have it: lazy binding, the call would abort the process)."""
    import subprocess
    stub = _stub_library(tmp_path, 3)
    src = tmp_path / "host.cpp"
    src.write_text('#include <cstdio>\n#include "fft_wgpu.hpp"\n'
                   'int main() {\n'
                   '  int caught = 0;\n'
                   '  try { fft_wgpu::Device d(0); } catch (const fft_wgpu::Error &e) { caught += e.status == FWA_ERR_UNSUPPORTED; std::puts(e.what()); }\n'
                   '  try { (void)fft_wgpu::enumerate_devices(); } catch (const fft_wgpu::Error &e) { caught += e.status == FWA_ERR_UNSUPPORTED; }\n'
                   '  return caught == 2 ? 0 : 1;\n}\n')
    exe = tmp_path / "host"
    # linked against the real library (every symbol resolves at link time), run against the stub (lazy binding: only the
    # functions actually called are looked up)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-L" + os.path.join(ROOT, "fft_wgpu_amd"), "-lfft_wgpu_amd", "-pthread", "-Wl,-z,lazy", "-o", str(exe)])
    r = subprocess.run([str(exe)], env=dict(os.environ, LD_LIBRARY_PATH=str(stub.parent)), capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    assert "ABI version 3" in r.stdout and "version 4" in r.stdout


def test_rust_shim_checks_the_abi_version_and_the_header_documents_the_ipc_mode():
    """Item 3 (a) and (c): the Rust mirror refuses a library of another version where the reference's prepare_gpu answers
    None (src/lib.rs:29-62); hosts of fwa_comm_* are told about HSA_ENABLE_IPC_MODE_LEGACY=0 in the header, in
    INTEGRATION.md and -- when RCCL fails without it -- in the error text."""
    ffi = open(os.path.join(ROOT, "rust_shim", "src", "ffi.rs")).read()
    helper = open(os.path.join(ROOT, "rust_shim", "src", "wgpu_helper.rs")).read()
    assert "ABI version 4" in ffi.split("\n")[0] and "pub const FWA_ABI_VERSION: i32 = 4;" in ffi
    body = helper[helper.index("pub fn open(ordinal: i32) -> Option<Device>"):]
    assert body.index("fwa_abi_version()") < body.index("fwa_ctx_create") and "return None" in body[:body.index("fwa_ctx_create")]
    header = open(os.path.join(ROOT, "include", "fft_wgpu_amd.h")).read()
    comm_block = header[header.index("multi-GPU: batch sharding"):header.index("typedef struct fwa_comm")]
    assert "HSA_ENABLE_IPC_MODE_LEGACY=0" in comm_block and "BEFORE the HIP runtime" in comm_block
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "HSA_ENABLE_IPC_MODE_LEGACY=0" in integration
    comm = open(os.path.join(ROOT, "fft_wgpu_amd", "csrc", "comm.cpp")).read()
    assert 'getenv("HSA_ENABLE_IPC_MODE_LEGACY")' in comm and "ipc_mode_hint()" in comm[comm.index("ncclCommInitRank"):]
