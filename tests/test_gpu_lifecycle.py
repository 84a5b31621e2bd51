"""GPU lifecycle tests (pytest -m gpu): network handles across call sequences — shape walks, pass order, weight re-upload, embedding slots, several
handles in one context, precision switches, batch walks, no allocation once warm, two sampler runs on the same objects (tests/lifecycle_checks.py).
Every pass is strict against the oracle (`relu-flips` for the ReLU tower's input gradient only) AND bit-equal to the same call on a fresh handle
in a fresh context."""
import pytest

from tests import lifecycle_checks as lc

pytestmark = pytest.mark.gpu


def _assert_all(recs, allowed=("strict",)):
    print("\n".join(f"{'ok  ' if r['ok'] else 'FAIL'} {r['name']}: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e} [{r['criterion']}]" for r in recs))
    bad = [r for r in recs if not r["ok"]]
    assert recs and not bad, "; ".join(f"{r['name']} [{r['criterion']}]: abs {r['err_abs']:.3e} rel {r['err_rel']:.3e} peak {r['ref_max']:.3e}"
                                       + (" VACUOUS" if r.get("vacuous") else "") for r in bad)
    assert all(r["criterion"] in allowed for r in recs), [r["name"] for r in recs if r["criterion"] not in allowed]


@pytest.mark.parametrize("precision", [1, 0])
def test_unet_shape_walk_and_no_allocation_once_warm(precision):
    _assert_all(lc.check_unet_shape_walk(precision))


def test_unet_cfg64_batch_walk():
    _assert_all(lc.check_unet_cfg64_walk())


def test_order_of_passes():
    _assert_all(lc.check_pass_order())


@pytest.mark.parametrize("kind", ["unet", "vit", "text", "rn", "lpips"])
def test_weight_reupload(kind):
    _assert_all(lc.check_reupload(kind), allowed=("strict", "relu-flips") if kind == "rn" else ("strict",))


def test_embedding_slots():
    _assert_all(lc.check_embed_slots())


def test_several_handles_in_one_context():
    _assert_all(lc.check_shared_context(), allowed=("strict", "relu-flips"))


def test_precision_switch_on_a_live_context():
    _assert_all(lc.check_precision_switch())


def test_tower_batch_walks_and_no_allocation_once_warm():
    _assert_all(lc.check_tower_walks(), allowed=("strict", "relu-flips"))


def test_two_sampler_runs_on_the_same_objects():
    _assert_all(lc.check_two_runs())


def test_classic_unet_shape_walk_and_no_allocation_once_warm():
    _assert_all(lc.check_classic_walk())


def test_classic_unet_pass_order_reupload_and_precision_switch():
    _assert_all(lc.check_classic_order_reupload_and_precision())


def test_classic_and_published_unet_interleaved_in_one_context():
    _assert_all(lc.check_classic_shared_context())
