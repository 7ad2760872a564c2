"""The steps of the BGZF compressor (besst_amd/csrc/bgzf_deflate_core.h: tokens, limited code lengths, the dynamic header,
the lanes' bit writer) run on the host, lane after lane, by tests/cpp/bgzf_deflate_core_test.cpp: every block it makes goes
through zlib's raw inflate on its own.  Compiled with the host C++ compiler, linked with zlib (which the library
itself links: csrc/build.sh) and run; its exit status is the verdict.  No GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for name in (os.environ.get('CXX'), 'c++', 'g++', 'clang++', '/opt/rocm/llvm/bin/clang++'):
        path = shutil.which(name) if name else None
        if path:
            return path
    raise AssertionError('no host C++ compiler found (set CXX)')


def test_bgzf_deflate_core_program(tmp_path):
    exe = str(tmp_path / 'bgzf_deflate_core_test')
    src = os.path.join(ROOT, 'tests', 'cpp', 'bgzf_deflate_core_test.cpp')
    built = subprocess.run([_host_compiler(), '-std=c++17', '-O1', '-Wall', '-Wextra', src, '-lz', '-o', exe], capture_output=True,
                           text=True)
    assert built.returncode == 0 and not built.stderr.strip(), built.stderr      # (a warning fails it too)
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, (ran.stdout + ran.stderr)[-3000:]
