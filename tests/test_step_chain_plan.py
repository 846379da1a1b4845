"""The ordering decisions of a step's chain, on the CPU: tests/host/step_chain_check.cpp compiles launch_plan.h and sfm.h (for
the two helpers that move the crowd's array sets) for the host.

plan_side_wiring over serial x sharded x 4096 / 4097 local robots x side_reads_all x remote_only x early step, plan_snap_turn and
plan_snap_in over early x listed x five sequence numbers with the wrap, plan_norm_chain's 16 cases and plan_crowd_step's 24, each
against a table written by hand from the code the functions replaced -- not printed from them.  Two model runs: the snapshots'
turns across the wrap (an early step never reads the buffer its own chain writes; a listed launch writes both and takes no turn),
and 4 x 400 steps of the crowd a step ahead with resets scattered by a fixed seed, where every launch ahead must wait for an event
recorded at or after the caller's stream's last access to the set it writes and last write to the set it reads -- with a wrong
rule beside it that the model has to catch.

The same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "step_chain_check.cpp")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    # (sfm.h keeps host-and-device helpers static that this program does not call)
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    return out.stdout.split()


def test_step_chain_decisions_and_models(tmp_path):
    words = _build_and_run(tmp_path, "step_chain_check", [])
    assert int(words[1]) > 10000  # (the checks ran: the crowd's model alone makes several per step)


def test_step_chain_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "step_chain_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
