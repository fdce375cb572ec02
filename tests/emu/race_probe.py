"""Builds and runs the schedules' probe (tests only): tests/emu/race_probe_main.cpp, a stand-alone host program linked against
the emulator library of tests/emu/emu.py for the fiber scheduler, with the emulator's SANITIZE flags.  It is started as a child
process with the schedule in its environment and prints one line per routine and form."""
import os
import subprocess

from . import emu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SRC = os.path.join(_HERE, "race_probe_main.cpp")
_BIN = os.path.join(_HERE, "race_probe_main")
_CSRC = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "circkit_amd", "csrc")


def build():
    base = emu.build()
    deps = [_SRC, base, os.path.join(_HERE, "wave_prims_emu.h"), os.path.join(_CSRC, "wave_prims.h")]
    if not os.path.exists(_BIN) or any(os.path.getmtime(d) > os.path.getmtime(_BIN) for d in deps):
        # the same UBSan + bounds flags as the emulator library, no recovery
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17"] + emu.SANITIZE + ["-o", _BIN, _SRC, "-L" + _HERE, "-l:libcanon_emu.so",
                              "-Wl,-rpath,$ORIGIN"])
    return _BIN


def run(schedule=None, timeout=120):
    """{(routine, "synced" | "unsynced"): [values]} under `schedule` (None: the environment's, ascending when unset)."""
    r = subprocess.run([build()], capture_output=True, text=True, timeout=timeout, env=emu.child_env(schedule))
    assert r.returncode == 0, "race_probe_main failed (%d): %s" % (r.returncode, r.stderr[-2000:])
    out = {}
    for line in r.stdout.splitlines():
        name, form, n, *values = line.split()
        assert len(values) == int(n)
        out[(name, form)] = [int(v) for v in values]
    return out


def run_skip(k, schedule=None, timeout=60):
    """(return code, stdout, stderr) of the workgroup in which somebody skips a collective (race_probe_main --skip k)."""
    r = subprocess.run([build(), "--skip", str(int(k))], capture_output=True, text=True, timeout=timeout, env=emu.child_env(schedule))
    return r.returncode, r.stdout, r.stderr
