"""CPU test: the run-time -> compile-time routing of csrc/sc_dispatch.hpp, in a stand-alone host program (tests/cpp/dispatch_routing.cpp)
built with the address and undefined-behaviour sanitizers.  No GPU, no kernel, no HIP header: only launch() needs the runtime."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispatch_header_routes_every_id_and_both_storage_types(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "dispatch_routing")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "dispatch_routing.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dispatch routing ok" in r.stdout
