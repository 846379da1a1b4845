"""What imgenv_create decides without a device, on the CPU: tests/host/create_plan_check.cpp compiles create_plan.h and out_fields.h
(and through them host_tables.h and launch_plan.h) for the host.

The arena: every offset and the total for a full handle of 4 robots (state_dim 3, 48 x 48 view = image, 181 beams, 3 pedestrians),
the same with IMGENV_FLAG_AGENT_STATE_EXTRAS, and a shard of 3 of 8 robots without laser and pedestrians, against literals DERIVED
BY HAND from the arithmetic plan_arena spelled out before the catalogue existed -- not printed from it; multiples of 256, no two
arrays overlapping, empty arrays on a slot of their own, the 32 names in order, `records` alone unguarded, the three extras alone
conditional.  The class layer's mode and the SUM word's bit budget (fits, past 32 bits, a shard's 64-cell box, the two flags), the
sub-steps of step_hz 0.4 / 0.1 / 0.05, the early-observation rule over all 256 corners, every refusal with its text character for
character (the world-cell limit in both wordings), and the smaller facts of a plan.

The same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "create_plan_check.cpp")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    # (host_tables.h keeps its table builders static, this program calls only a few; fp_rows.h carries a device-side unroll pragma)
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Werror", "-Wno-unused-function", "-Wno-unknown-pragmas", "-ffp-contract=off"] + flags + [SOURCE, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    return out.stdout.split()


def test_create_plan_arena_layer_refusals(tmp_path):
    words = _build_and_run(tmp_path, "create_plan_check", [])
    assert int(words[1]) > 1000  # (the checks ran: the three arenas alone make over 700)


def test_create_plan_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "create_plan_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
