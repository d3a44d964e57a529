"""CPU: host-side logic of the drop-in C++ headers (samplers, PROSAC order, inlier index lists) compiled with g++ and run.
The program only links the C-ABI library for the symbols the headers reference; it makes no GPU call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_logic_cpp(tmp_path):
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "host_logic")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "host_logic.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "host_logic: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_lie_group_properties_cpp(tmp_path):
    """rpe::SO3 / rpe::SE3 of the drop-in headers against the properties sophus/tests.hpp:43-198 checks (exp vs the matrix exponential,
    action, product, inverse), Tp = double and float."""
    from rgbd_pose_estimation_amd import build
    lib = build.build()
    exe = str(tmp_path / "lie_properties")
    inc = os.path.join(ROOT, "rgbd_pose_estimation_amd", "include")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", os.path.join(inc, "pose"), "-I", inc,
                           os.path.join(ROOT, "tests", "cpp", "lie_properties.cpp"), "-L", os.path.dirname(lib), "-lrgbdpose_hip",
                           "-Wl,-rpath," + os.path.dirname(lib), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lie_properties: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_resident_slot_policy_cpp(tmp_path):
    """Who waits for whom on the GPU's one resident slot (round-5 advisor finding: sessions held it across calls and everybody else
    blocked without a time-out): loops wait for loops, never for sessions; sessions wait for sessions at most until the holder's grid
    has left, then take over; a revoked holder finds out and its release is a no-op.  hipcc-compiled host program, no HIP call."""
    import shutil
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "resident_slot")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-Wall", "-Wno-unused-function", "-x", "hip",
                           os.path.join(ROOT, "tests", "cpp", "resident_slot.cpp"), "-lpthread", "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "resident_slot: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_device_buffer_cpp(tmp_path):
    """rpeh::DevBuf, the one owner of plain device memory in the host units (csrc/rpe_devbuf.hpp), against a fake runtime over
    malloc / free: reserve / once, the all-or-nothing regrow with a failure injected at every malloc, copy and the wait, moves inside a
    std::vector.  g++ with AddressSanitizer (leak detection on) and UBSan; a stand-alone program that links no HIP runtime."""
    exe = str(tmp_path / "devbuf_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "devbuf_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "devbuf_host: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


def test_gn_host_cpp(tmp_path):
    """The Gauss-Newton step, the round loop and the coarse-to-fine walk every host loop of the library runs (csrc/rpe_gn_host.hpp) on
    scripted rounds and levels: round counts under tol and at max_iter, a loop taken up part way, a refused system, a round's own error,
    the cost scale, level order, gates, the fine level, an error at a level, the argument complaints.  g++ with AddressSanitizer and
    UBSan; a stand-alone program that links neither the library nor the HIP runtime."""
    exe = str(tmp_path / "gn_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "gn_host.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0 and "gn_host: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
