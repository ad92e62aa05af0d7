"""Option "nn" of a tic-tac-toe ctx where there is no GPU: "device" is refused with DIEE_ERR_HIP and the ctx goes on working on the host."""
import numpy as np
import pytest
import torch

import diee_amd

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="a GPU is present: tests/test_ttt_device_gpu.py covers the option")


def test_device_network_without_a_gpu_is_refused_and_the_ctx_stays_on_the_host():
    blob = diee_amd.random_weights(0, diee_amd.GAME_TTT)
    eng, fresh = diee_amd.Engine(0, diee_amd.GAME_TTT), diee_amd.Engine(0, diee_amd.GAME_TTT)
    eng.load_weights(blob); fresh.load_weights(blob)
    assert eng.get_option("nn") == "host"
    with pytest.raises(diee_amd.DieeError) as ei:
        eng.set_option("nn", "device")
    assert ei.value.status == diee_amd.ERR_HIP and "GPU" in str(ei.value)
    assert eng.get_option("nn") == "host"
    states = diee_amd.ttt_new(5)
    states["board"] = np.random.default_rng(1).integers(-1, 2, size=(5, 9))
    (p, v), (fp, fv) = eng.forward_t(states), fresh.forward_t(states)
    assert p.tobytes() == fp.tobytes() and v.tobytes() == fv.tobytes()
    with pytest.raises(diee_amd.DieeError) as ei:
        eng.set_option("compact", 0)
    assert ei.value.status == diee_amd.ERR_UNSUPPORTED
    with pytest.raises(diee_amd.DieeError) as ei:
        eng.set_option("nn", "fast")
    assert ei.value.status == diee_amd.ERR_ARG
    eng.close(); fresh.close()
