"""Option "search_fused" of a tic-tac-toe ctx that searches on the host: "1" is refused with DIEE_ERR_ARG (the key is known: not
DIEE_ERR_UNSUPPORTED) and the ctx goes on searching as a fresh one does."""
import pytest
import torch

import diee_amd

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="a GPU is present: tests/test_ttt_fused_gpu.py covers the option")


def test_fused_search_on_a_host_ctx_is_refused_and_the_ctx_searches_on():
    blob = diee_amd.random_weights(0, diee_amd.GAME_TTT)
    eng, fresh = diee_amd.Engine(0, diee_amd.GAME_TTT), diee_amd.Engine(0, diee_amd.GAME_TTT)
    eng.load_weights(blob); fresh.load_weights(blob)
    with pytest.raises(diee_amd.DieeError) as ei:
        eng.set_option("search_fused", "1")
    assert ei.value.status == diee_amd.ERR_ARG and "search" in str(ei.value)
    assert eng.get_option("search_fused") == "0" and eng.get_option("search_last_launches") == "0"
    assert int(eng.get_option("search_fused_lds_iters")) >= 50
    roots, cfg = diee_amd.ttt_new(3), diee_amd.MctsConfig.default(10)
    a, b = eng.alpha_mcts_parallel(roots, cfg, 5, 2), fresh.alpha_mcts_parallel(roots, cfg, 5, 2)
    assert a["probs"].tobytes() == b["probs"].tobytes() and a["root_visits"].tobytes() == b["root_visits"].tobytes()
    eng.close(); fresh.close()
