"""What an enable call of an optional feature decides before it touches a device, on the CPU: tests/host/feature_plan_check.cpp
compiles img_env_amd/csrc/feature_plan.h and the slot catalogue of obs_fields.h for the host.

The refusals: every code and text feature_plan.h can return, against literals copied from the FAIL lines the enable functions had
before the header existed.  Their order: a cfg refusal in front of the null handle, the IMGENV_*_NORM_* bits in front of the null
handle, the prerequisites behind the repeated call where that was the order (the policy head, the loss, obs_post, the field
features) and in front of it where that was (the episode log, the minibatches).  The same-cfg predicates: a copy compares equal,
every compared member makes a cfg differ, the others do not.  The catalogue: for the final observations, the rollout and the
minibatches, the selected fields in block order and the member each pointer lands in, with every optional array and with none,
against the three lists the enable functions used to spell out; the silent skip and the refusal.

The same program runs once more under AddressSanitizer and UndefinedBehaviorSanitizer, as a program of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "host", "feature_plan_check.cpp")


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O0", "-std=c++17", "-Wall", "-Werror"] + flags + [SOURCE, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    return out.stdout.split()


def test_feature_plan_refusals_order_predicates_and_catalogue(tmp_path):
    words = _build_and_run(tmp_path, "feature_plan_check", [])
    assert int(words[1]) > 600  # (the checks ran: the refusals alone make more than 300, the catalogue as many again)


def test_feature_plan_under_sanitizers(tmp_path):
    _build_and_run(tmp_path, "feature_plan_check_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
