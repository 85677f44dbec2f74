"""The test suite's own support modules, on the CPU: the by-name caller every GPU launch of
tests/launches.py goes through refuses what it must (a fake library: nothing is launched), the
tree comparison of tests/pop_support.py reports what differs and where, and the net-kind table
of launches.device_epoch covers mlp_ref's epoch case."""
import pytest
import torch

import launches
import mlp_ref as R
from abi_args import by_name, declared
from pop_support import differences, equal_tree, same

FN = "nav_grad_reduce"


class FakeLib:
    """An entry point that records its positional arguments and returns a chosen status."""

    def __init__(self, status=0):
        self.status, self.got = status, None

    def nav_grad_reduce(self, *args):
        self.got = args
        return self.status


def _valid():
    return {name: i for i, name in enumerate(declared(FN))}


def test_by_name_passes_the_arguments_in_the_headers_order():
    assert declared(FN) == ["net", "hidden_slabs", "splits", "edge_slabs", "edge_blocks", "grad",
                            "stream"]
    lib = FakeLib()
    by_name(lib, FN, **_valid())
    assert lib.got == tuple(range(7))
    # a header name Python keeps for itself is spelled as abi_args.SPELLED says
    assert "inp" in declared("nav_mlp_wgrad") and "in" not in declared("nav_mlp_wgrad")


@pytest.mark.parametrize("what", ["missing", "surplus", "misordered"])
def test_by_name_refuses_other_keywords(what):
    args = _valid()
    if what == "missing":
        del args["splits"]
    elif what == "surplus":
        args["ld"] = 0
    else:
        args = {k: args[k] for k in ["hidden_slabs", "net"] + declared(FN)[2:]}
    lib = FakeLib()
    with pytest.raises(AssertionError):
        by_name(lib, FN, **args)
    assert lib.got is None  # refused before anything was passed


def test_by_name_refuses_a_non_zero_status():
    with pytest.raises(AssertionError):
        by_name(FakeLib(status=-100000), FN, **_valid())


def _tree():
    return {"a": torch.arange(4.0), "n": 3, "l": [torch.zeros(2), 7],
            "d": {"x": torch.ones(2), "y": {"z": torch.tensor([1, 2])}}}


def test_differences_reports_the_paths():
    a, b = _tree(), _tree()
    assert differences(a, b) == [] and same(a, b)
    equal_tree(a, b)
    b["a"][2] = -1.0                      # a tensor
    b["n"] = 4                            # a scalar
    b["l"][1] = 8                         # inside a list
    b["d"]["y"]["z"] = torch.tensor([1, 3])  # inside a nested tree
    assert differences(a, b, "root") == ["root/a", "root/n", "root/l/1", "root/d/y/z"]
    assert not same(a, b)
    with pytest.raises(AssertionError, match="root/a"):
        equal_tree(a, b, "root")
    # NaN is no NaN: the comparison is torch.equal's
    assert differences({"t": torch.tensor([float("nan")])}, {"t": torch.tensor([float("nan")])})


def test_differences_asserts_on_another_shape_of_tree():
    a, b = _tree(), _tree()
    b["l"].append(0)
    with pytest.raises(AssertionError, match="/l"):
        differences(a, b)
    b = _tree()
    del b["d"]["y"]["z"]
    with pytest.raises(AssertionError, match="/d/y"):
        differences(a, b)


def test_kind_table_covers_the_epoch_case():
    assert set(launches.KIND) == set(R.EPOCH_SEEDS)
    for name in R.EPOCH_SEEDS:
        want = (2, 2) if name in ("ta", "actor", "atgt") else (4, 1)
        assert launches.KIND[name] == want, name
    # and the case's layers have those shapes
    case = R.epoch_case(24, 1, 4)
    for name, layers in case["layers"].items():
        d_in, d_out = launches.KIND[name]
        assert layers[0][0].shape[1] == d_in and layers[-1][0].shape[0] == d_out, name
    assert case["ring"] == R.RING == case["rows"].shape[0]
