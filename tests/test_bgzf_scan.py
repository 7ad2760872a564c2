"""The host side of the device ingest that reads file bytes with hand-written bounds - the BGZF header walk, the boundary
search, the part cut, the chunk plan (besst_amd/csrc/bgzf_scan.h) - on hand-made blocks: tests/cpp/bgzf_scan_test.cpp is
compiled with the host C++ compiler and run; its exit status is the verdict.  No GPU."""
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


def test_bgzf_scan_program(tmp_path):
    exe = str(tmp_path / 'bgzf_scan_test')
    src = os.path.join(ROOT, 'tests', 'cpp', 'bgzf_scan_test.cpp')
    built = subprocess.run([_host_compiler(), '-std=c++17', '-O1', '-Wall', '-Wextra', src, '-o', exe], capture_output=True, text=True)
    assert built.returncode == 0 and not built.stderr.strip(), built.stderr      # (a warning fails it too)
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert ran.returncode == 0, ran.stdout + ran.stderr
