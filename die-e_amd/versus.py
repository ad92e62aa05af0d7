"""Arena: the second caller of the hot path.  Mirrors the reference's
src/versus.rs: play() (:160-268), get_actions_for_player (:270-318), Game JSON save / load / replay
(:27-122).  Model agents search on the HIP engine (diee_mcts_batch), and so does the Mcts agent (vanilla UCB1 with
rollouts, diee_mcts_vanilla_batch): by default the reference's agent as written, whose rollout plays nothing (node.rs:181,
Q22); DIEE_VANILLA_ROLLOUTS=1 (or vanilla_rollouts=True) turns the quirk off -- opt-in and logged, like the project's other deviations.

`play` is written against a small backend interface so that the same driver can run on the engine or,
in the parity tests, on the CPU oracle.  `play_device` is the same arena as ONE engine call (diee_arena): every round
on the device, the same games bit for bit (Model, Mcts and Random agents); DIEE_ARENA=device makes the callers use it.

The reference declares Turn { roll, action, player } and Game.turns, and print_game walks them, but play() never pushes one (Q21).
record_turns=True (DIEE_RECORD_TURNS=1 for `diee.py play`) is the replay as it was meant -- opt-in and logged: both drivers record
every turn with the two fields that make it replayable (next_roll, is_second_play), replay_states re-plays and audits a recorded
game, print_game shows the board after each turn.
"""
import json
import os
import secrets
import sys

import numpy as np

from . import BG_ACTIONS, BG_STATE, NO_MOVE

TAG_INIT_ROLL, TAG_MOVE_ROLL, TAG_SAMPLE = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD
START = [2, 0, 0, 0, 0, -5, 0, -3, 0, 0, 0, 5, -5, 0, 0, 0, 3, 0, 5, 0, 0, 0, 0, -2]   # backgammon_logic.rs:83-88


class Agent:                                   # versus.rs:17-20
    RANDOM, MCTS, MODEL, NONE = "Random", "Mcts", "Model", "None"

    @staticmethod
    def parse(s):                              # main.rs:126-144
        m = {"model": Agent.MODEL, "mcts": Agent.MCTS, "random": Agent.RANDOM}
        if s is None or s.lower() not in m:
            raise ValueError("Incorrect specification for agent's type.")
        return m[s.lower()]


class Player:                                  # versus.rs:124-127
    def __init__(self, player_type, model=None):
        self.player_type, self.model = player_type, model


class EngineRules:
    """rules / RNG / arithmetic served by the HIP engine (any engine instance will do)"""

    def __init__(self, engine):
        self.e = engine

    def valid_moves(self, states):
        return self.e.get_valid_moves(states)

    def apply(self, states, plays, dice):
        return self.e.apply_move(states, plays, dice)

    def decode(self, states, codes):
        return self.e.decode(states, codes)

    def powf(self, x, y):
        return self.e.det_pow(x, y)

    def draws(self, seed, ctr):
        return self.e.probe_dice(seed, ctr)     # (dice [n,2], uniform [n])


class EngineSearch:
    """alpha_mcts_parallel + get_prob_tensor_parallel on an engine loaded with one player's weights"""

    def __init__(self, engine):
        self.e = engine

    def mcts(self, states, cfg, seed, step, ids, rounds):
        r = self.e.alpha_mcts_parallel(states, cfg, seed, step, ids, rounds, ref_quirks=True)
        return r["probs"], r["n_children"]

    def vanilla(self, states, cfg, seed, ids, rounds, ref_quirks):
        """mct_search per game (Agent::Mcts) -> plays int8 [n,4]; needs no weights"""
        return self.e.mct_search(states, cfg, seed, ids, rounds, ref_quirks=ref_quirks)["plays"]


def vanilla_rollouts_from_env(log=None):
    """DIEE_VANILLA_ROLLOUTS=1: the Mcts agent's rollouts are played (the reference's Q22 off), opt-in and logged"""
    on = os.environ.get("DIEE_VANILLA_ROLLOUTS") == "1"
    if on:
        (log or (lambda m: sys.stderr.write(m + "\n")))("[diee] DIEE_VANILLA_ROLLOUTS=1: Agent::Mcts plays its rollouts "
                                                        "(deviation from the reference, whose simulate() returns 0: Q22)")
    return on


def record_turns_from_env(log=None):
    """DIEE_RECORD_TURNS=1: saved games carry their turns (the reference never fills Game.turns: Q21), opt-in and logged"""
    on = os.environ.get("DIEE_RECORD_TURNS") == "1"
    if on:
        (log or (lambda m: sys.stderr.write(m + "\n")))("[diee] DIEE_RECORD_TURNS=1: games are saved with their turns, each with next_roll and "
                                                        "is_second_play (deviation from the reference, whose play() pushes no turn: Q21)")
    return on


def turn_json(roll, play, player, next_roll, second):
    """Turn { roll, action, player } (versus.rs:21-26) as JSON, plus what makes it replayable: action = the (from, to) pairs of the play,
    none for a skipped turn; player = the Agent that moved; next_roll = the dice apply_move / skip_turn was given"""
    p = [int(x) for x in play]
    return {"roll": [int(roll[0]), int(roll[1])], "action": [[p[i], p[i + 1]] for i in (0, 2) if p[i] != NO_MOVE], "player": player,
            "next_roll": [int(next_roll[0]), int(next_roll[1])], "is_second_play": bool(second)}


def new_states(n):
    s = np.zeros(n, dtype=BG_STATE)
    s["pts"] = START
    s["player"] = -1
    return s


def skip_turn(states, dice):                   # backgammon_logic.rs:192-196
    out = states.copy()
    out["second"] = 0
    out["player"] = -out["player"]
    out["roll"] = dice
    return out


def check_winner(states):                      # backgammon_logic.rs:527-534 (player -1 first)
    w = np.zeros(len(states), dtype=np.int8)
    w[states["off"][:, 1] == 15] = 1
    w[states["off"][:, 0] == 15] = -1
    return w


def weighted_select(row, u01):                 # alphazero.rs:129-137 (rand WeightedIndex over f64 weights)
    """cumulative weights in index order (sequential f64 sums, like the device code), u ~ U[0,total), first
    index whose cumulative weight exceeds u"""
    cum = np.cumsum(row.astype(np.float64))    # np.cumsum is a sequential running sum
    x = u01 * cum[-1]
    hit = np.nonzero(cum > x)[0]
    if len(hit):
        return int(hit[0])
    nz = np.nonzero(row)[0]
    return int(nz[-1]) if len(nz) else 0


class Game:                                    # versus.rs:27-52
    def __init__(self, player1, player2, state, idx):
        self.id = secrets.token_urlsafe(16)[:21]
        self.player1, self.player2 = player1, player2
        self.turns = []                        # never populated by the reference either (Q21)
        self.winner = Agent.NONE
        self.initial_state = {"board": [[int(x) for x in state["pts"]], [int(x) for x in state["bar"]],
                                        [int(x) for x in state["off"]]],
                              "roll": [int(x) for x in state["roll"]], "player": int(state["player"]),
                              "is_second_play": bool(state["second"]), "id": int(idx)}

    def to_json(self):
        return {"id": self.id, "player1": self.player1, "player2": self.player2, "turns": self.turns,
                "winner": self.winner, "initial_state": self.initial_state}


def save_game(game, game_path):                # versus.rs:54-63
    path = os.path.join(game_path, f"{game.id}.json")
    with open(path, "w") as f:
        json.dump(game.to_json(), f, indent=2)
    return path


def load_game(path):                           # versus.rs:65-73
    with open(path) as f:
        return json.load(f)


def to_pretty_str(st):                         # backgammon_logic.rs:110-174
    board = st["board"][0]
    bot = [str(i) for i in range(11, -1, -1)]
    top = [str(i) for i in range(12, 24)]

    def cell(i, n):
        if i == 6 and i <= abs(n):
            return f"+{abs(n) - 5}"
        if i <= abs(n):
            return "x" if n < 0 else "o"
        return " "
    inner = [[cell(i, board[p]) for p in range(11, -1, -1)] for i in range(1, 7)]
    inner.append([" "] * 12)
    inner += [[cell(i, board[p]) for p in range(12, 24)] for i in range(6, 0, -1)]
    rows = [bot] + inner + [top]
    for r in rows:
        r.insert(len(r) // 2, "|"); r.insert(0, "|"); r.append("|")
    body = "\n".join("\t".join(r) for r in reversed(rows))
    who = "Player 1" if st["player"] == -1 else "Player 2"
    info = (f"Current turn: {who}\tRoll: {tuple(st['roll'])}\n"
            f"Player 1:\n\tBroken Pieces: {st['board'][1][0]}\n\tPieces Collected:{st['board'][2][0]}\n"
            f"Player 2:\n\tBroken Pieces: {st['board'][1][1]}\n\tPieces Collected:{st['board'][2][1]}")
    bar = "=" * 110
    return f"{info}\n{bar}\n{body}\n{bar}"


def state_from_json(st):
    """Game.initial_state -> one BG_STATE record"""
    s = np.zeros(1, dtype=BG_STATE)
    s["pts"][0], s["bar"][0], s["off"][0] = st["board"][0], st["board"][1], st["board"][2]
    s["roll"][0], s["player"][0], s["second"][0] = st["roll"], st["player"], 1 if st["is_second_play"] else 0
    return s[0]


def apply_turn(st, turn):
    """the state (a dict like Game.initial_state) after a recorded turn, on the host: apply_move (backgammon_logic.rs:176-186, its moves by
    get_next_state, :467-517) or skip_turn (:192-196) with the turn's next_roll.  What print_game needs; nothing is checked here
    (replay_states checks a game against the rules)"""
    pts, bar, off = (list(x) for x in st["board"])
    player = st["player"]
    me = 0 if player < 0 else 1
    for f, t in turn["action"]:
        if t == -1:                            # collect
            pts[f] -= player; off[me] += 1
            continue
        hit = pts[t] == -player
        if f == -1:                            # from the bar
            bar[me] -= 1
        else:
            pts[f] -= player
        if hit:
            pts[t] += 2 * player; bar[1 - me] += 1
        else:
            pts[t] += player
    out = dict(st, board=[pts, bar, off])
    if turn["action"] and st["roll"][0] == st["roll"][1] and not st["is_second_play"]:
        out["is_second_play"] = True           # the second half of a double: same side, same roll
    else:
        out.update(roll=list(turn["next_roll"]), player=-player, is_second_play=False)
    return out


def replay_all(games, rules):
    """replay_states for several games at once (one rules call per turn index for all of them)"""
    docs = [g.to_json() if isinstance(g, Game) else g for g in games]
    cur = np.array([state_from_json(d["initial_state"]) for d in docs], dtype=BG_STATE).reshape(len(docs))
    outs = [np.zeros(len(d["turns"]), dtype=BG_STATE) for d in docs]
    for t in range(max([len(d["turns"]) for d in docs], default=0)):
        act = np.array([i for i, d in enumerate(docs) if t < len(d["turns"])])
        sub = cur[act]
        vm, cnt = rules.valid_moves(sub)
        plays = np.full((len(act), 4), NO_MOVE, dtype=np.int8)
        dice = np.zeros((len(act), 2), dtype=np.uint8)
        for k, i in enumerate(act):
            d, turn = docs[i], docs[i]["turns"][t]
            where = f"game {d['initial_state']['id']} ({d['id']}), turn {t}: "
            if "next_roll" not in turn:
                raise ValueError(where + "the record has no next_roll (not recorded by this project: nothing to replay)")
            if [int(x) for x in sub[k]["roll"]] != list(turn["roll"]):
                raise ValueError(where + f"recorded roll {turn['roll']}, the state's is {[int(x) for x in sub[k]['roll']]}")
            if bool(sub[k]["second"]) != bool(turn["is_second_play"]):
                raise ValueError(where + f"recorded is_second_play {turn['is_second_play']}, the state's is {bool(sub[k]['second'])}")
            mover = d["player1"] if sub[k]["player"] == -1 else d["player2"]
            if turn["player"] != mover:
                raise ValueError(where + f"recorded player {turn['player']}, to move is {mover}")
            flat = [x for pair in turn["action"] for x in pair]
            if not flat:
                if mover in (Agent.RANDOM, Agent.MCTS) and cnt[k] != 0:
                    raise ValueError(where + f"a skipped turn of a {mover} agent with {int(cnt[k])} legal plays")
            else:
                if len(flat) not in (2, 4):
                    raise ValueError(where + f"action {turn['action']} is not one or two (from, to) pairs")
                plays[k, :len(flat)] = flat
                if not (vm[k][:cnt[k]] == plays[k]).all(axis=1).any():
                    raise ValueError(where + f"action {turn['action']} is not a valid move")
            dice[k] = turn["next_roll"]
        empty = plays[:, 0] == NO_MOVE
        new = sub.copy()
        if empty.any():
            new[empty] = skip_turn(sub[empty], dice[empty])
        if (~empty).any():
            new[~empty] = rules.apply(sub[~empty], plays[~empty], dice[~empty])
        cur[act] = new
        for k, i in enumerate(act):
            outs[i][t] = new[k]
    return outs


def replay_states(game, rules):
    """the state after every turn of a recorded game (a Game or its JSON), by rules.apply / skip_turn with the recorded dice -> BG_STATE
    [len(turns)].  Audits the record on the way: every turn's roll, is_second_play and player against the state, every action against
    rules.valid_moves, and that a Random or Mcts agent skipped only without a legal play; ValueError on the first mismatch, naming the
    game and the turn"""
    return replay_all([game], rules)[0]


def print_game(path, wait_user_input=False, out=print):     # versus.rs:75-105
    g = load_game(path)
    out(f"Game ID: {g['id']}")
    out(f"Player 1: {g['player1']}, Player 2: {g['player2']}")
    out(f"Game winner: {g['winner']}")
    out("Initial State:")
    out(to_pretty_str(g["initial_state"]))
    state = g["initial_state"]
    for turn in g["turns"]:
        out(f"Player: {turn['player']}"); out(f"Roll: {turn['roll']}"); out(f"Action: {turn['action']}")
        if "next_roll" in turn:                # a turn this project recorded: the two lines versus.rs:92-93 comment out
            state = apply_turn(state, turn)
        out("State after action has been played:"); out(to_pretty_str(state))
        if wait_user_input:
            input("Press Enter to continue...")


class PlayResult:                              # versus.rs:129-152
    def __init__(self, player1, player2, wins_p1, wins_p2, n_games, games):
        self.player1, self.player2, self.wins_p1, self.wins_p2 = player1, player2, wins_p1, wins_p2
        self.n_games, self.games = n_games, games
        self.draws = n_games - (wins_p1 + wins_p2)
        self.winrate = wins_p1 / n_games       # from p1's perspective

    def __str__(self):
        return (f"Player 1: {self.player1}\nPlayer 2: {self.player2}\nWins Player 1: {self.wins_p1}\n"
                f"Wins Player 2: {self.wins_p2}\nDraws: {self.draws}\nNumber of Games: {self.n_games}\n"
                f"Winrate: {self.winrate * 100.}%\n")


def get_actions_for_player(player, states, ids, rnd, mcts_config, temp, seed, rules, search, side, vanilla_quirks=True):
    """versus.rs:270-318 -> plays int8 [n,4] (all NO_MOVE = EMPTY_MOVE)"""
    n = len(states)
    plays = np.full((n, 4), NO_MOVE, dtype=np.int8)
    if n == 0:
        return plays
    ctr = np.stack([ids, np.full(n, rnd), np.full(n, TAG_SAMPLE), np.zeros(n)], axis=1).astype(np.uint32)
    _, uni = rules.draws(seed, ctr)
    if player.player_type == Agent.MODEL:
        probs, nch = search.mcts(states, mcts_config, seed, 2 * rnd + side, ids.astype(np.uint32),
                                 np.full(n, rnd, dtype=np.uint32))
        inv_t = np.float32(1.0 / float(temp))
        codes = np.full(n, 1351, dtype=np.uint32)
        ri, ci = np.nonzero(np.nan_to_num(probs) > 0)
        powed = np.zeros((n, BG_ACTIONS), dtype=np.float32)
        if len(ri):
            powed[ri, ci] = rules.powf(probs[ri, ci].astype(np.float32), inv_t)  # .pow_(1.0 / temp), :283 (one batched call)
        for i in range(n):
            if nch[i] == 0 or float(powed[i].sum()) == 0.0:   # :292 all-zero row (e.g. iterations = 0) or root.children.is_empty() -> EMPTY_MOVE
                continue
            codes[i] = weighted_select(powed[i], float(uni[i]))
        return rules.decode(states, codes)     # :301
    if player.player_type == Agent.RANDOM:     # :308-317
        vm, cnt = rules.valid_moves(states)
        for i in range(n):
            if cnt[i]:
                plays[i] = vm[i][min(int(uni[i] * cnt[i]), cnt[i] - 1)]
        return plays
    if search is None:
        raise NotImplementedError("Agent::Mcts (vanilla MCTS with rollouts) runs on the engine: give the player an engine (Player.model) "
                                  "or pass a search object with .vanilla()")
    # :303-306 mct_search per game (the drawn uniform is not used)
    return np.asarray(search.vanilla(states, mcts_config, seed, ids.astype(np.uint32), np.full(n, rnd, dtype=np.uint32), vanilla_quirks),
                      dtype=np.int8).reshape(n, 4)


def play(player1, player2, mcts_config, temp, seed=0xD1EE0001, num_games=400, round_limit=400, rules=None,
         search1=None, search2=None, max_rounds=0, vanilla_rollouts=None, record_turns=False):
    """play(), versus.rs:160-268.  player1 plays side -1 in every game; the second half of the games starts
    with side +1 to move (:172-174).  max_rounds > 0 stops the loop after that many rounds (the games still alive
    are not in `games`); 0 plays to the end.  An Mcts player searches on its engine (Player.model) or on search1 / search2;
    vanilla_rollouts: its rollouts are played (Q22 off); None reads DIEE_VANILLA_ROLLOUTS.  record_turns: every Game's `turns` is filled (Q21)
    and PlayResult.turns holds them for every game index, retired or not."""
    if vanilla_rollouts is None:
        vanilla_rollouts = Agent.MCTS in (player1.player_type, player2.player_type) and vanilla_rollouts_from_env()
    if rules is None:
        eng = player1.model or player2.model
        if eng is None:
            raise ValueError("an engine is needed for the rules (pass rules=...)")
        rules = EngineRules(eng)
    if search1 is None and player1.player_type == Agent.MODEL:
        search1 = EngineSearch(player1.model)
    if search2 is None and player2.player_type == Agent.MODEL:
        search2 = EngineSearch(player2.model)
    if search1 is None and player1.player_type == Agent.MCTS and player1.model is not None:
        search1 = EngineSearch(player1.model)
    if search2 is None and player2.player_type == Agent.MCTS and player2.model is not None:
        search2 = EngineSearch(player2.model)

    states = new_states(num_games)
    idx = np.arange(num_games)
    ctr = np.stack([idx, np.zeros(num_games), np.full(num_games, TAG_INIT_ROLL), np.zeros(num_games)], axis=1).astype(np.uint32)
    dice, _ = rules.draws(seed, ctr)
    states["player"][num_games // 2:] = 1      # skip_turn() for idx >= num_games/2 (its roll is overwritten by roll_die, Q23)
    states["roll"] = dice
    games = [Game(player1.player_type, player2.player_type, states[i], i) for i in range(num_games)]
    alive = np.ones(num_games, dtype=bool)
    wins_p1 = wins_p2 = 0
    played = []
    round_count = 0
    while alive.any() and (max_rounds == 0 or round_count < max_rounds):      # :191
        live = np.nonzero(alive)[0]
        p1 = live[states["player"][live] == -1]  # :195-196 partition by side to move
        p2 = live[states["player"][live] != -1]
        acts = {}
        for side, (pl, ids, srch) in enumerate(((player1, p1, search1), (player2, p2, search2))):
            a = get_actions_for_player(pl, states[ids], ids, round_count, mcts_config, temp, seed, rules, srch, side,
                                       vanilla_quirks=not vanilla_rollouts)
            for k, g in enumerate(ids):
                acts[int(g)] = a[k]
        rnd = round_count
        round_count += 1                       # :219
        order = np.concatenate([p1, p2])
        ctr = np.stack([order, np.full(len(order), rnd), np.full(len(order), TAG_MOVE_ROLL), np.zeros(len(order))],
                       axis=1).astype(np.uint32)
        dice, _ = rules.draws(seed, ctr)
        pl = np.stack([acts[int(g)] for g in order])
        if record_turns:                       # the turn as it is about to be played: the state's roll, the action, who moves, the dice it is given
            for k, g in enumerate(order):
                mover = player1.player_type if k < len(p1) else player2.player_type
                games[g].turns.append(turn_json(states[g]["roll"], pl[k], mover, dice[k], states[g]["second"]))
        empty = pl[:, 0] == NO_MOVE
        if empty.any():                        # :225-228 skip_turn; continue (no winner / round-limit check)
            states[order[empty]] = skip_turn(states[order[empty]], dice[empty])
        mv = ~empty
        if mv.any():
            sub = order[mv]
            vm, cnt = rules.valid_moves(states[sub])
            for k in range(len(sub)):          # :229 assert!(valid_moves.contains(action))
                assert (vm[k][:cnt[k]] == pl[mv][k]).all(axis=1).any(), "decoded action is not a valid move"
            states[sub] = rules.apply(states[sub], pl[mv], dice[mv])
            win = check_winner(states[sub])
            for k, g in enumerate(sub):
                w = int(win[k]) if win[k] != 0 else (0 if round_count >= round_limit else None)   # :233-237
                if w is None:
                    continue
                alive[g] = False
                if w == -1:
                    games[g].winner = player1.player_type; wins_p1 += 1
                elif w == 1:
                    games[g].winner = player2.player_type; wins_p2 += 1
                else:
                    games[g].winner = Agent.NONE
                played.append(games[g])
    res = PlayResult(player1.player_type, player2.player_type, wins_p1, wins_p2, num_games, played)
    res.final_states = states
    res.rounds = round_count
    res.turns = [g.turns for g in games] if record_turns else None
    return res


def retired_order(winner, retired_round, retired_side):
    """the order in which play() appends the games it retires: by round, within a round player 1's list before player 2's, within a
    list by game index -> indices of the retired games (retired_round 0xFFFFFFFF = still alive: left out)"""
    rr = np.asarray(retired_round, dtype=np.uint32)
    done = np.nonzero(rr != 0xFFFFFFFF)[0]
    side = np.asarray(retired_side)[done].astype(np.int64)
    return done[np.lexsort((done, side, rr[done].astype(np.int64)))]


def games_from_device(player1, player2, initial_states, winner, retired_round, retired_side):
    """play()'s `games` from the per-game outputs of Engine.arena"""
    names = {-1: player1.player_type, 1: player2.player_type, 0: Agent.NONE}
    games = []
    for g in retired_order(winner, retired_round, retired_side):
        game = Game(player1.player_type, player2.player_type, initial_states[g], g)
        game.winner = names[int(winner[g])]
        games.append(game)
    return games


def play_device(player1, player2, mcts_config, temp, seed=0xD1EE0001, num_games=400, round_limit=400, max_rounds=0, engine=None,
                vanilla_rollouts=None, record_turns=False):
    """play() with every round on the device (Engine.arena, diee_arena): the same PlayResult -- wins, draws, rounds, final_states,
    games in play()'s order -- from one engine call.  Model, Mcts and Random agents; `engine` hosts a call none of whose players brings an
    engine.  vanilla_rollouts as in play(): the Mcts agent's searches run without the quirks, a Model agent's with them (a flag word per
    player, diee_arena_ex).  record_turns: Game.turns and PlayResult.turns from the device's turn log, the same turns play() records."""
    from . import AGENT_MCTS, AGENT_MODEL, AGENT_RANDOM, FLAG_REF_QUIRKS, arena
    kinds = {Agent.MODEL: AGENT_MODEL, Agent.RANDOM: AGENT_RANDOM, Agent.MCTS: AGENT_MCTS}
    types = (player1.player_type, player2.player_type)
    if vanilla_rollouts is None:
        vanilla_rollouts = Agent.MCTS in types and vanilla_rollouts_from_env()
    # the quirks per player, as play() searches: a Model agent always with them, an Mcts agent without them when its rollouts are played
    quirks = [not (vanilla_rollouts and t == Agent.MCTS) for t in types]
    for s in (0, 1):
        if types[s] == Agent.RANDOM:           # (a Random agent searches nothing: the other player's word)
            quirks[s] = quirks[1 - s]
    e1, e2 = player1.model, player2.model
    if e1 is None and e2 is None:
        e1 = engine                            # no player brings an engine (Random, Mcts): any engine hosts the call
    r = arena(e1, kinds[player1.player_type], e2, kinds[player2.player_type], num_games, mcts_config, temp, seed, round_limit, max_rounds,
              ref_quirks=quirks[0], record_turns=record_turns,
              flags2=None if quirks[0] == quirks[1] else (FLAG_REF_QUIRKS if quirks[1] else 0))
    games = games_from_device(player1, player2, r["initial_states"], r["winner"], r["retired_round"], r["retired_side"])
    turns = None
    if record_turns:
        names = {v: k for k, v in kinds.items()}
        rec, first = r["turns"], r["first"].tolist()
        roll, pl, agent, nxt, second = (rec[k].tolist() for k in ("roll", "play", "agent", "next_roll", "second"))     # (Python ints: the lists are long)
        turns = [[turn_json(roll[i], pl[i], names[agent[i]], nxt[i], second[i]) for i in range(first[g], first[g + 1])] for g in range(num_games)]
        for game in games:
            game.turns = turns[game.initial_state["id"]]
    res = PlayResult(player1.player_type, player2.player_type, r["wins_p1"], r["wins_p2"], num_games, games)
    res.final_states = r["final_states"]
    res.rounds = r["rounds"]
    res.turns = turns
    res.device = r                             # the call's per-game outputs and per-player stats
    return res


# ---- the same arena for tic-tac-toe (play::<TicTacToe>, versus.rs:160-268 is generic over LearnableGame) ------------------
def play_tictactoe(player1, player2, mcts_config, temp, seed=0xD1EE0001, num_games=400, round_limit=400):
    """Model / Random agents on the tic-tac-toe host engine (BASELINE configs[0]); player1 plays side -1 in every game, the
    second half of the games starts after a skip_turn() (:172-174), a draw (check_winner = Some(0)) has no winner"""
    from . import TTT_ACTIONS, ttt_apply_move, ttt_check_winner, ttt_new, ttt_valid_moves
    states = ttt_new(num_games)
    states["player"][num_games // 2:] = 1
    alive = np.ones(num_games, dtype=bool)
    wins_p1 = wins_p2 = 0
    round_count = 0
    rules_eng = player1.model or player2.model
    while alive.any():
        live = np.nonzero(alive)[0]
        sides = (live[states["player"][live] == -1], live[states["player"][live] != -1])
        acts = {}
        for side, (pl, ids) in enumerate(((player1, sides[0]), (player2, sides[1]))):
            if len(ids) == 0:
                continue
            # the sampling uniforms: the engine's Philox stream (seed, game, round, TAG_SAMPLE); tic-tac-toe has no dice
            uni = np.array([_uniform01(seed, int(g), round_count) for g in ids])
            if pl.player_type == Agent.MODEL:
                r = pl.model.alpha_mcts_parallel(states[ids], mcts_config, seed, 2 * round_count + side, ids.astype(np.uint32),
                                                 np.full(len(ids), round_count, dtype=np.uint32), ref_quirks=True)
                inv_t = np.float32(1.0 / float(temp))
                for k, g in enumerate(ids):
                    if r["n_children"][k] == 0:
                        continue                                                      # EMPTY_MOVE, versus.rs:292
                    row = np.nan_to_num(r["probs"][k]).astype(np.float32)
                    nz = row > 0
                    powed = np.zeros(TTT_ACTIONS, dtype=np.float32)
                    powed[nz] = np.power(row[nz].astype(np.float64), float(inv_t)).astype(np.float32)   # .pow_(1.0 / temp), :283
                    if float(powed.sum()) == 0.0:
                        continue                                                      # `prob_tensor.sum() == 0` -> EMPTY_MOVE too, versus.rs:286-293
                    acts[int(g)] = weighted_select(powed, float(uni[k]))
            elif pl.player_type == Agent.RANDOM:
                for k, g in enumerate(ids):
                    vm = ttt_valid_moves(states[g])
                    if vm:
                        acts[int(g)] = vm[min(int(uni[k] * len(vm)), len(vm) - 1)]
            else:
                raise NotImplementedError("Agent::Mcts (vanilla MCTS with rollouts) runs on the backgammon engine only; the tic-tac-toe "
                                          "Mcts agent is not provided")
        round_count += 1                                                                 # :219
        for g in np.concatenate(sides):
            g = int(g)
            if g not in acts:                                                            # :225-228 skip_turn; continue
                states[g]["player"] = -states[g]["player"]
                continue
            assert acts[g] in ttt_valid_moves(states[g]), "decoded action is not a valid move"       # :229
            states[g] = ttt_apply_move(states[g], acts[g])
            w = ttt_check_winner(states[g])
            if w is None and round_count >= round_limit:
                w = 0                                                                    # :235
            if w is None:
                continue
            alive[g] = False
            wins_p1 += w == -1; wins_p2 += w == 1
    res = PlayResult(player1.player_type, player2.player_type, int(wins_p1), int(wins_p2), num_games, [])
    res.final_states = states
    res.rounds = round_count
    return res


def _uniform01(seed, game, rnd):
    """draw_uniform of csrc/bg_device.h (Philox4x32-10 keyed by seed / game / round / TAG_SAMPLE) on the host, for the arena's
    sampling of a game without an engine-side draw entry point"""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    k0, k1 = seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF
    c = [game & 0xFFFFFFFF, rnd & 0xFFFFFFFF, TAG_SAMPLE, 0]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & 0xFFFFFFFF, p1 & 0xFFFFFFFF, ((p0 >> 32) ^ c[3] ^ k1) & 0xFFFFFFFF, p0 & 0xFFFFFFFF]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    x = (c[3] << 32) | c[2]
    return (x >> 11) * (1.0 / 9007199254740992.0)
