"""Option "arena_last_launches" of a tic-tac-toe ctx (the search-kernel launches of its last diee_ttt_arena on the device) on a host ctx:
known, read-only and 0."""
import pytest

import diee_amd


def test_arena_last_launches_on_a_host_ctx():
    e = diee_amd.Engine(0, diee_amd.GAME_TTT)
    assert e.get_option("arena_last_launches") == "0"
    R = diee_amd.AGENT_RANDOM
    assert e.ttt_arena(R, None, R, 4, diee_amd.MctsConfig.default(4), flags=[0, 0])["rounds"] >= 5
    assert e.get_option("arena_last_launches") == "0"                       # the host loop launches nothing
    with pytest.raises(diee_amd.DieeError) as ei:
        e.set_option("arena_last_launches", "1")
    assert ei.value.status == diee_amd.ERR_ARG                              # read-only, not unknown
    e.close()
