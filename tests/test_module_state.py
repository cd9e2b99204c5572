"""The module registry of vx_ctx and dev_grow (vx_host.inl), checked on the host: tests/cpp/module_state_test.cpp includes what
the CPU emulation includes, registers stand-in module states and verifies creation on first use, peek, a failed set-up, and
that destroying the context drops every created state once, in the order of the enum."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_module_registry_and_dev_grow(tmp_path):
    exe = str(tmp_path / "module_state_test")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-Wno-unknown-pragmas", "-Wno-subobject-linkage", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "module_state_test.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "OK", out.stdout + out.stderr
