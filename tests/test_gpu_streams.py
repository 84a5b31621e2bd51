"""GPU stream tests (pytest -m gpu): every entry on a created, non-blocking stream behind a pending delay (tests/stream_checks.py).  Each
case is bit-equal to its control on the default stream, leaves its inputs alone and — once warm — returns to the host while the delay is
still running; the harness is first shown to catch a launch on the null stream, a synchronising call and a call that writes nothing."""
import pytest
import torch as th

from tests import stream_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def prepared():
    """every case built, warmed and controlled once; the delay fixed from the measured host times; the premise asserted"""
    st = sc.prepare()
    print("\n" + sc.report())
    v = st["premise"]
    assert v.early and not v.problems(), f"premise: a pure-torch trial must return early and match its control: {v.problems()}"
    return st


def _assert_all(recs, allowed=("strict",)):
    print("\n".join(f"{'ok  ' if r['ok'] else 'FAIL'} {r['name']}: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e} [{r['criterion']}]" for r in recs))
    bad = [r for r in recs if not r["ok"]]
    assert recs and not bad, "; ".join(f"{r['name']} [{r['criterion']}]: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e} peak {r['ref_max']:.3e}"
                                       + (" VACUOUS" if r.get("vacuous") else "") for r in bad)
    assert all(r["criterion"] in allowed for r in recs), [r["name"] for r in recs if r["criterion"] not in allowed]


# ---- the detector must be shown to detect ------------------------------------------------------------------------------------------------
def _operand():
    a = th.randn(4096, generator=sc.g(7)).to(sc.DEV)
    th.cuda.synchronize()
    return a


def test_detector_catches_a_launch_on_the_null_stream():
    def fake(a):
        with th.cuda.stream(th.cuda.default_stream()):
            return a * 2

    v = sc.behind_delay(fake, [_operand()], warm=True, name="fake: torch op on the default stream")
    print(v.problems())
    assert not v.equal[0][0], ("a launch on the null stream was NOT caught: it waited for the delay on the created stream, so on this machine "
                               "the two streams are ordered with each other (they may share a hardware queue) and this whole tier is "
                               "vacuous here")
    assert v.equal[0][1], "the output of the early launch holds poison (NaN)"


def test_detector_catches_a_synchronising_call():
    def fake(a):
        out = a * 2
        th.cuda.current_stream().synchronize()
        return out

    v = sc.behind_delay(fake, [_operand()], warm=True, name="fake: synchronises the current stream")
    print(v.problems())
    assert v.early is False and v.equal[0][0]
    assert any("did not return" in p for p in v.problems())


def test_detector_catches_a_call_that_writes_nothing():
    v = sc.behind_delay(lambda a: th.empty_like(a), [_operand()], warm=True, name="fake: writes nothing",
                        ref=(_operand() * 2,))
    print(v.problems())
    assert not v.equal[0][0] and v.equal[0][1], "the untouched output is still NaN"


# ---- cases -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sc.CASES))
def test_entry_behind_a_delay_on_a_created_stream(name):
    # `relu-flips`: the input gradient of the two ReLU networks against their oracle, as everywhere else in the suite
    _assert_all(sc.run_case(name), allowed=("strict", "relu-flips") if name.startswith(("resnet", "secondary model")) else ("strict",))


@pytest.mark.parametrize("kind", ["unet", "vit"])
def test_forward_and_dgrad_on_two_streams(kind):
    _assert_all(sc.check_handover(kind))


def test_two_networks_alternating_on_two_streams_through_one_context():
    _assert_all(sc.check_alternating())


def test_groupnorm_records_are_served_to_the_producing_stream_only():
    _assert_all(sc.check_records_across_streams())


@pytest.mark.parametrize("dtype", [th.float16, th.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("kind", sc.UPLOAD_KINDS)
def test_weight_upload_from_a_state_dict_built_on_the_stream(kind, dtype):
    _assert_all(sc.check_upload(kind, dtype))


@pytest.mark.parametrize("kind,source", [("unet", "device"), ("unet", "cpu"), ("rn", "device"), ("rn", "cpu"), ("text", "device")])
def test_weight_reupload_while_a_pass_is_in_flight(kind, source):
    _assert_all(sc.check_reupload_in_flight(kind, source))


def test_three_guided_ddim_steps_entirely_on_a_created_stream():
    recs = sc.check_guided_run()
    print("early per step:", sc._STATE.get("guided_run_early"))
    _assert_all(recs)
