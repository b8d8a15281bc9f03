"""The strip kernel's schedule on the CPU: csrc/tic_strip_plan.h holds the launcher's plan and the function the kernel's prologue calls to find a
wave's first strip; tests/native/strip_plan_selftest.cpp (a stand-alone program, g++ -fsanitize=address,undefined) walks every workgroup and
wave of a set of frames with them."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_strip_plan_visits_every_strip_once(tmp_path):
    """Per frame and schedule: every strip of the fast rectangle exactly once, every offset inside the frame and that of the strip the walk is
    at, at most 64 strips per wave, idle waves on strip 0, the division-free cursor equal to the schedule's general form.  Frames: one strip;
    72x16 aligned and not; one strip row; 1920x1080 (the cursor wraps inside a walk); the smallest 2048-wide frame on the team schedule (found
    by the plan's own rule: 2048x1536) with one block row fewer and one more; three frames with a gap; 512x512, 1920x1080 and 4096x4096 on
    64 workgroups under each TIC_SCHED; eight rounds; 16384x16384; 256 x 1080p.  The program's `broken` mode (the kernel told of one strip
    fewer than the plan covers) must fail."""
    exe = tmp_path / "strip_plan_selftest"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "strip_plan_selftest.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("strip_plan_selftest ok"), r.stdout[-3000:] + r.stderr[-3000:]
    assert "smallest 2048-wide frame on the team schedule: 2048x1536" in r.stdout and "no fast rectangle" in r.stdout
    for kind in ("rows (team)", "chunk,", "round,"):
        assert kind in r.stdout, kind
    b = subprocess.run([str(exe), "broken"], capture_output=True, text=True, timeout=120)
    assert b.returncode == 1 and "strip_plan_selftest FAILED" in b.stdout and "strips missed" in b.stdout, b.stdout[-3000:] + b.stderr[-3000:]
