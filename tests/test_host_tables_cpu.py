"""CPU: the host-side tables of the forward chains (csrc/host_tables.hpp: LRU table, environment switch, statistics read-out),
checked by a stand-alone program (host_tables_main.cpp, next to this file) built with the address and undefined-behaviour
sanitizers and run as a child process.  The header includes nothing from HIP, so plain g++ builds it."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_host_tables_under_sanitizers(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "host_tables_main")
    # the sanitizer runtimes are linked INTO the program: it then runs whatever else the environment loads ahead of its libraries
    r = subprocess.run([cxx, "-std=c++17", "-fsanitize=address,undefined", "-static-libasan", "-static-libubsan",
                        "-fno-sanitize-recover=all", "-g", "-Wall", "-Werror",
                        os.path.join(HERE, "host_tables_main.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "host tables ok" in r.stdout
