"""The self-play host's measured window and scheduler as programs of their own, under sanitizers; nothing is loaded into
Python.  tools/measure_window_check.cpp feeds p3achygo_amd/host/measure_window.h (the single definition of the benchmark's
timed region) scripted completion sequences under the address and undefined-behaviour sanitizers;
tools/selfplay_tsan_main.cpp runs the scheduler (lanes, spare rows, straggler hand-over) under ThreadSanitizer, built by
the host Makefile's tsan_check target."""
import os
import re
import shutil
import subprocess

from conftest import ROOT


def test_window_on_scripted_completions_under_sanitizers(tmp_path):
    """steps, rounds (late reports on both sides of t0 and t1), the advance phase, failed runs, the least-squares fit and
    the seconds limit: every expectation is derived by hand beside its sequence in the program"""
    cxx = shutil.which("g++")
    assert cxx, "g++ is needed to build the window's sanitizer program"
    exe = str(tmp_path / "measure_window_check")
    # the sanitizer runtimes are linked statically: the program does not care what else the loader brings in, and the
    # child runs in the environment it inherits
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                    os.path.join(ROOT, "tools", "measure_window_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines[-1] == "ok" and int(lines[-2].split()[0]) >= 90, run.stdout


def test_window_header_needs_nothing_else_of_the_host():
    """the check program includes measure_window.h alone, and that header only the game counters"""
    src = open(os.path.join(ROOT, "tools", "measure_window_check.cpp")).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["../p3achygo_amd/host/measure_window.h"]
    hdr = open(os.path.join(ROOT, "p3achygo_amd", "host", "measure_window.h")).read()
    assert re.findall(r'#include "([^"]+)"', hdr) == ["game_stats.h"]
    assert "::now()" not in hdr and "std::thread" not in hdr


def test_scheduler_under_thread_sanitizer(tmp_path):
    """two groups x two lanes, four playouts in flight, 128 games on 4 threads, slow games: 12 rounds without a report,
    and host phases did hand stragglers over"""
    make = shutil.which("make")
    assert make and shutil.which("g++"), "make and g++ are needed to build the scheduler's ThreadSanitizer program"
    run = subprocess.run([make, "-C", os.path.join(ROOT, "p3achygo_amd", "host"), "-j8", "tsan_check", f"TSAN_DIR={tmp_path}"],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-4000:] + run.stderr[-4000:]
    assert "ThreadSanitizer" not in run.stdout + run.stderr
    m = re.search(r"rc 0: (\d+) batches, 12 rounds, .* handed over: (\d+) phases, (\d+) games\nok\n", run.stdout)
    assert m and int(m.group(1)) >= 12 and int(m.group(2)) > 0 and int(m.group(3)) >= int(m.group(2)), run.stdout[-2000:]
