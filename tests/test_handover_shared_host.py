"""The pieces every device hand-over shares, with no GPU: the destination-row check of the store ops on
host tensors, the budget loop with stub sets, and the life cycle of the two ``from_st`` datasets on device 'cpu' with an
explicit byte budget (nothing asks a GPU for its free memory)."""
import types

import numpy as np
import pytest
import torch

DEV = torch.device("cuda:0")              # only compared with: a host ``dst`` is checked where it lies


# ----------------------------------------------------------------------------- the row check
def test_row_check_accepts_distinct_rows_and_repeated_skips():
    from egaze_amd.hipops import check_rows
    check_rows(torch.tensor([[0, 1, 2], [3, 4, 5]]), (2, 3), DEV, "late_store", "plane")
    check_rows(torch.tensor([4, 0, 2]), (3,), DEV, "lstm_store", "row")
    check_rows(torch.tensor([[0, -1, -1], [-1, -1, -1]]), (2, 3), DEV, "late_store", "plane")
    check_rows(torch.tensor([-1, -1, 7, -1]), (4,), DEV, "lstm_store", "row")


def test_row_check_refuses_a_repeat_naming_the_first():
    from egaze_amd.hipops import check_rows
    with pytest.raises(ValueError, match=r"late_store: dst names plane 4 twice"):      # 4 repeats before 0 does
        check_rows(torch.tensor([[0, 4, 2], [4, 0, 5]]), (2, 3), DEV, "late_store", "plane")
    with pytest.raises(ValueError, match=r"lstm_store: dst names row 2 twice"):
        check_rows(torch.tensor([2, -1, 2]), (3,), DEV, "lstm_store", "row")


def test_row_check_refuses_another_type_or_shape():
    from egaze_amd.hipops import check_rows
    with pytest.raises(ValueError, match="int64"):
        check_rows(torch.tensor([0, 1], dtype=torch.int32), (2,), DEV, "lstm_store", "row")
    with pytest.raises(ValueError, match=r"\(2, 3\)"):
        check_rows(torch.tensor([[0, 1, 2]]), (2, 3), DEV, "late_store", "plane")
    with pytest.raises(ValueError, match=r"\(2,\)"):
        check_rows(torch.tensor([0]), (2,), DEV, "lstm_store", "row")
    with pytest.raises(ValueError, match="contiguous"):
        check_rows(torch.tensor([[0, 1], [2, 3], [4, 5]]).t(), (2, 3), DEV, "late_store", "plane")
    with pytest.raises(ValueError, match="int64"):
        check_rows([0, 1], (2,), DEV, "lstm_store", "row")


def test_row_check_counts_only_the_columns_it_is_given():
    from egaze_amd.hipops import check_rows
    dst = torch.tensor([[0, 1, 7], [3, 4, 7]])            # the third column is not written through without a gt_pool
    check_rows(dst, (2, 3), DEV, "late_store", "plane", cols=2)
    with pytest.raises(ValueError, match="plane 7 twice"):
        check_rows(dst, (2, 3), DEV, "late_store", "plane")
    with pytest.raises(ValueError, match="plane 3 twice"):
        check_rows(torch.tensor([[0, 3, 7], [3, 4, 8]]), (2, 3), DEV, "late_store", "plane", cols=2)


# ----------------------------------------------------------------------------- the budget loop
def _stubs(*needs):
    return [types.SimpleNamespace(needed_bytes=n, name=k) for k, n in enumerate(needs)]


def test_a_total_over_the_budget_raises_before_any_set_is_touched():
    from egaze_amd.data.resident import under_budget
    calls = []
    with pytest.raises(RuntimeError, match="need 101, 100 allowed"):
        under_budget(_stubs(60, 41), 100, lambda needed, budget: f"need {needed}, {budget} allowed",
                     lambda ds, left: calls.append((ds.name, left)))
    assert calls == []


def test_a_total_equal_to_the_budget_passes_and_the_remainder_is_handed_down():
    from egaze_amd.data.resident import under_budget
    calls = []
    under_budget(_stubs(60, 30, 10), 100, lambda needed, budget: "refused", lambda ds, left: calls.append((ds.name, left)))
    assert calls == [(0, 100), (1, 40), (2, 10)]          # each set is handed what the ones before it left: the last fits exactly


def test_budget_in_gb_less_what_is_spent():
    from egaze_amd.data.resident import resident_budget
    assert resident_budget("cuda:0", 0.5) == 500000000
    assert resident_budget("cuda:0", 0.5, spent=123) == 500000000 - 123
    assert resident_budget("cuda:0", 1e-3, spent=2000000) == -1000000      # nothing left: every set is refused


# ----------------------------------------------------------------------------- the life cycle of the from_st sets
def _late_set():
    from egaze_amd.data.late_resident import ResidentLateDataset
    names = [f"Ahmad_Pizza1_img_{k:05d}.png" for k in range(10, 14)]
    gts = [f"Ahmad_Pizza1_000000_{k:05d}.png" for k in range(10, 14)]
    st = types.SimpleNamespace(listTrainFiles=names, listGtFiles=gts, gtPath="gt", hw=(6, 10))
    return ResidentLateDataset.from_st(st)


def _lstm_set():
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    names = [f"Ahmad_Pizza1_img_{k:05d}.png" for k in range(10, 18)]
    st = types.SimpleNamespace(listTrainFiles=names, fixsac=np.array([1, 1, 0, 0, 1, 1, 1, 0], dtype=float))
    return ResidentLSTMDataset.from_st(st)


@pytest.mark.parametrize("make, beside", [(_late_set, "table"), (_lstm_set, "plan")])
def test_allocate_mark_filled_filled(make, beside):
    ds = make()
    assert ds._handover and not ds._complete and ds.pool is None and not ds.filled
    with pytest.raises(RuntimeError, match=r"mark_filled: allocate\(device\) has not run"):
        ds.mark_filled()
    assert not ds.filled
    with pytest.raises(RuntimeError, match=rf"{ds.needed_bytes} bytes.* {ds.needed_bytes - 1} bytes are allowed"):
        ds.allocate("cpu", budget_bytes=ds.needed_bytes - 1)
    assert ds.pool is None and getattr(ds, beside) is None and not ds.filled
    assert ds.allocate("cpu", budget_bytes=ds.needed_bytes) is ds          # a set that needs exactly the budget fits
    assert ds.pool is not None and not bool(ds.pool.any()) and getattr(ds, beside) is not None
    assert not ds.filled and not ds._complete
    assert ds.mark_filled() is ds and ds.filled and ds._complete
    ds.allocate("cpu", budget_bytes=ds.needed_bytes)                        # a new pool is empty again
    assert not ds.filled
    with pytest.raises(RuntimeError, match=r"fill: a from_st set has no files"):
        ds.fill("cpu")


def test_shapes_of_what_allocate_creates():
    late, lstm = _late_set().allocate("cpu", budget_bytes=1 << 20), _lstm_set().allocate("cpu", budget_bytes=1 << 20)
    assert late.pool.dtype == torch.uint8 and tuple(late.pool.shape) == (12, 6, 10) and torch.equal(late.table, late.plane_table)
    assert lstm.pool.dtype == torch.float32 and tuple(lstm.pool.shape) == (2, 512)
    assert [tuple(p.shape) for p in lstm.plan] == [(0,)] * 3               # two vectors: no step


def test_the_lstm_sets_release_clears_filled():
    ds = _lstm_set().allocate("cpu", budget_bytes=1 << 20).mark_filled()
    assert ds.filled
    ds.release()
    assert ds.pool is None and ds.plan is None and not ds.filled and not ds._complete
    with pytest.raises(RuntimeError, match="mark_filled"):
        ds.mark_filled()
    ds.allocate("cpu", budget_bytes=1 << 20)
    assert not ds.filled                                   # ... and a pool allocated after it starts incomplete


def test_allocate_on_a_file_backed_set_raises(tmp_path):
    from egaze_amd.data.late_resident import ResidentLateDataset
    from egaze_amd.data.lstm_resident import ResidentLSTMDataset
    folder = tmp_path / "vec"
    folder.mkdir()
    for k in range(3):
        torch.save(torch.zeros(512), str(folder / f"fix_Ahmad_Pizza1_img_{10 + k:05d}.pth.tar"))
    listed = ResidentLSTMDataset(str(folder))
    with pytest.raises(RuntimeError, match=r"ResidentLSTMDataset.allocate: only a from_st set is allocated empty; fill\(\) reads"):
        listed.allocate("cpu", budget_bytes=1 << 20)
    assert listed.pool is None and not listed.filled and not listed._handover
    names = ["a.png", "b.png"]
    late = ResidentLateDataset("pred", "gt", "feat", names, names, names)
    with pytest.raises(RuntimeError, match=r"ResidentLateDataset.allocate: only a from_st set is allocated empty; fill\(\) decodes"):
        late.allocate("cpu", budget_bytes=1 << 20)
    assert late.pool is None and not late.filled and not late._handover
