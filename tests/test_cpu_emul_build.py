"""The build rule of the host emulation libraries (tests/emul_build.py) against what the compiler says they read: every
file `g++ -MM` names for a library's main source and -D switches has to be in the rule's dependency set, and a library
older than the newest of them has to count as stale -- a CPU tier that passes on yesterday's library guards nothing."""
import os
import subprocess

import pytest

from tests import emul_build as eb

NO_HANDOVER = ["-DRAYS_RK4_NO_HANDOVER"]
# every (main source, -D switches) the CPU tier builds a library from (the -D variants of a library read the same files)
LIBRARIES = {
    "trace": ("emul_trace.cpp", []),
    "probe": ("emul_probe.cpp", []),
    "group": ("emul_group.cpp", []),
    "summary": ("emul_summary.cpp", NO_HANDOVER),
    "summary_wave": ("emul_summary.cpp", NO_HANDOVER + ["-DRAYS_EMUL_SUMMARY_WAVE=1"]),
    "window": ("emul_window.cpp", NO_HANDOVER),
    "window_wave": ("emul_window.cpp", NO_HANDOVER + ["-DRAYS_EMUL_WINDOW_WAVE=1"]),
    "fused": ("emul_fused_deposition.cpp", NO_HANDOVER),
    "fused_wave": ("emul_fused_deposition.cpp", NO_HANDOVER + ["-DRAYS_EMUL_DEPOSIT_WAVE=1"]),
}


def _reads(src, defs):
    """The files inside the repository that the preprocessor opens for this build."""
    cmd = [a for a in eb.command(src, "unused.so", defs) if a != "-shared"]
    rule = subprocess.check_output(cmd[:-2] + ["-MM"], text=True)
    files = [os.path.realpath(f) for f in rule.split(":", 1)[1].replace("\\\n", " ").split()]
    return [f for f in files if f.startswith(os.path.realpath(eb.ROOT) + os.sep)]


@pytest.mark.parametrize("name", sorted(LIBRARIES))
def test_build_rule_covers_what_the_library_reads(name, tmp_path):
    src, defs = LIBRARIES[name]
    reads = _reads(src, defs)
    deps = {os.path.realpath(f) for f in eb.dependencies()}
    assert os.path.realpath(os.path.join(eb.DIR, src)) in reads and len(reads) > 10, reads
    assert not [f for f in reads if f not in deps], "read by the library, unknown to tests/emul_build.py"
    # the staleness rule itself, on stand-ins with set mtimes: the newest file the library reads is the newest of all
    stand_ins = []
    for k, f in enumerate(sorted(deps)):
        stand_ins.append(str(tmp_path / f"dep{k}"))
        open(stand_ins[-1], "w").close()
        os.utime(stand_ins[-1], (1000, 1000))
    newest = stand_ins[sorted(deps).index(max(reads, key=os.path.getmtime))]
    os.utime(newest, (2000, 2000))
    lib = str(tmp_path / "lib.so")
    assert eb.stale(lib, stand_ins)   # no library yet
    open(lib, "w").close()
    os.utime(lib, (1999, 1999))
    assert eb.stale(lib, stand_ins)
    os.utime(lib, (2000, 2000))
    assert not eb.stale(lib, stand_ins)
    os.utime(lib, (2001, 2001))
    assert not eb.stale(lib, stand_ins)
