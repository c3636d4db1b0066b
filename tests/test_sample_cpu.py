"""ops.sample semantics on hand-written rows (reference path, CPU) and the
sampling fields of the serving engine on llama-tiny."""
import pytest
import torch

from kubeflow_amd import ops
from kubeflow_amd.ops import reference
from kubeflow_amd.runtime.serving import InferenceEngine, Request

NINF = float("-inf")
PLATEAU = [2.0, 2.0, 1.0, 1.0, 1.0, 0.0, NINF]
# masses at temperature 1: 1, 1, e^-1 (x3), e^-2, 0 -> prefixes in rank
# order 1, 2, 2.368, 2.736, 3.104, 3.239

CASES = {
    # top_k = 3 cuts the plateau of ones by index: 0..2 stay, 2 is the last
    "topk_plateau_last": (PLATEAU, 1.0, 3, 1.0, 0.999, 2),
    "topk_plateau_mid": (PLATEAU, 1.0, 3, 1.0, 0.5, 1),
    # top_p = 0.8 of 3.239 is 2.591: reached inside the plateau, at index 3
    "topp_plateau_last": (PLATEAU, 1.0, 0, 0.8, 0.999, 3),
    "topp_below_top_mass": (PLATEAU, 1.0, 0, 0.2, 0.999, 0),
    "greedy_lowest_index": ([1.0, 3.0, 3.0, 2.0], 0.0, 2, 0.5, 0.9, 1),
    "u_zero_first_kept": ([NINF, 1.0, 2.0], 1.0, 0, 1.0, 0.0, 1),
    # k = 4 is above the two finite entries: the -inf ones are never drawn
    "ninf_never_drawn": ([1.0, NINF, NINF, 0.0, NINF], 1.0, 4, 1.0, 0.999, 3),
    "ninf_all_greedy": ([NINF, NINF, NINF], 1.0, 0, 1.0, 0.5, 0),
    "nan_ranks_last": ([float("nan"), -5.0, NINF], 0.0, 0, 1.0, 0.0, 1),
}


@pytest.mark.parametrize("case", CASES)
def test_hand_written_rows(case):
    row, temperature, k, p, u, want = CASES[case]
    args = (torch.tensor([row]), torch.tensor([temperature]),
            torch.tensor([k], dtype=torch.int32), torch.tensor([p]),
            torch.tensor([u]))
    assert reference.sample(*args, dtype=torch.float64).tolist() == [want]
    got = ops.sample(*args)
    assert got.dtype == torch.int32 and got.tolist() == [want]


@pytest.fixture(scope="module")
def engine():
    torch.manual_seed(0)
    eng = InferenceEngine("llama-tiny", max_slots=4, smax=256,
                          max_batch=4).start()
    yield eng
    eng.stop()


def test_fields_reach_request_and_top_k_1_is_greedy(engine):
    greedy = engine.generate([1, 2, 3], max_new_tokens=6)
    r = engine.generate([1, 2, 3], max_new_tokens=6, temperature=1.0,
                        top_k=1, top_p=0.5, seed=11)
    assert (r.top_k, r.top_p, r.seed, r.error) == (1, 0.5, 11, "")
    assert r.generated == greedy.generated


def test_seeded_request_ignores_its_batch(engine):
    """Seeds 3 / 4 / 5 at temperature 1.5: the request with seed 3 draws the
    same tokens alone and decoding next to the two others."""
    def request(seed, prompt):
        return Request(rid=f"s{seed}", prompt=prompt, max_new_tokens=8,
                       temperature=1.5, top_k=40, top_p=0.95, seed=seed)

    alone = engine.submit(request(3, [5, 6, 7]))
    assert alone.done.wait(120) and alone.error == ""
    batch = [engine.submit(request(s, p)) for s, p in
             ((4, [9, 8, 7]), (3, [5, 6, 7]), (5, [2, 4, 6]))]
    assert all(r.done.wait(120) and r.error == "" for r in batch)
    assert batch[1].generated == alone.generated
    assert len({tuple(r.generated) for r in batch}) == 3  # really sampled
