"""Option "search" of a tic-tac-toe ctx whose network is on the host: "device" is refused with DIEE_ERR_ARG and the ctx goes on searching on the host."""
import pytest
import torch

import diee_amd

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="a GPU is present: tests/test_ttt_search_gpu.py covers the option")


def test_device_search_over_the_host_network_is_refused_and_the_ctx_stays_on_the_host():
    blob = diee_amd.random_weights(0, diee_amd.GAME_TTT)
    eng, fresh = diee_amd.Engine(0, diee_amd.GAME_TTT), diee_amd.Engine(0, diee_amd.GAME_TTT)
    eng.load_weights(blob); fresh.load_weights(blob)
    assert eng.get_option("nn") == "host" and eng.get_option("search") == "host"
    with pytest.raises(diee_amd.DieeError) as ei:
        eng.set_option("search", "device")
    assert ei.value.status == diee_amd.ERR_ARG and "nn" in str(ei.value)
    assert eng.get_option("search") == "host"
    roots, cfg = diee_amd.ttt_new(3), diee_amd.MctsConfig.default(10)
    a, b = eng.alpha_mcts_parallel(roots, cfg, 5, 2), fresh.alpha_mcts_parallel(roots, cfg, 5, 2)
    assert a["probs"].tobytes() == b["probs"].tobytes() and a["root_visits"].tobytes() == b["root_visits"].tobytes()
    eng.close(); fresh.close()
