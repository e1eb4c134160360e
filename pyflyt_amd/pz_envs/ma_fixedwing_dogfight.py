"""PettingZoo-ParallelEnv-shaped façade of the team dogfight env
(pz_envs/fixedwing_envs/ma_fixedwing_dogfight_env.py:14-833, ma_fixedwing_base_env.py:17-408).

Same constructor keywords and defaults, agent naming ("uav_i", agents [0, team_size) one team, the rest the other),
dict-in / dict-out `reset()` / `step()`, the flattened observation [attitude 12, surfaces + throttle 6, health, past action 4] +
14 per other active aircraft (its attitude in the own body frame, health, same-team flag) zero padded, the accumulate-then-pop
rewards, culling of finished agents (their aircraft fly on with zero commands), infos (`health`, `received_hits`, `dead`,
`collision`, `out_of_bounds`, `team_win`). All aircraft of an env copy share one world (drone-drone collisions, contact
response on); the whole env step is ONE kernel launch (pyflyt_amd/csrc/dogfight.hpp).

Differences from the reference, by construction of the batched path:
  * `num_envs` independent copies of the whole multi-agent env are stepped at once: dict values are tensors of shape
    [num_envs, ...] (squeezed to the reference's per-agent vectors when num_envs == 1);
  * the spawn circle of every copy is drawn from the counter-based RNG (Philox keyed by seed and the copy's first lane), not
    from `np.random.RandomState(seed)`: the same distribution (:176-213), a different stream;
  * `flatten_observation=False`: the device always writes the flattened, zero-padded vector; the Dict form is a host-side
    view of it -- {"self": [23], "others": [k, 14]} with the k active others exactly as in the reference when num_envs == 1,
    and {"self": [E, 23], "others": [E, A - 1, 14] zero padded, "others_mask": [E, A - 1]} for num_envs > 1 (a Sequence
    space has no batched form);
  * `freeze_wrecks=True` (default False = the reference's behaviour) stops an aircraft where it hits the ground instead of
    letting it tumble to rest: it leaves the others' observations one update later, and the step time of a world with
    wrecks stays that of a world in flight (the contact solve of a tumbling airframe is the most expensive thing here);
  * `assisted_flight=False` does what the reference does with it: the action is six numbers wide, the Aviary stays in mode 0
    (ma_fixedwing_base_env.py:229) and reads the first four, entries 4 and 5 only show up in the observed past action, and the
    thrust remap lands on the unused sixth entry, so the thrust command is action[3] as given (pinned by a reference trajectory).
"""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib as L
from ..dist import strong_shard
from ..engine import BatchEngine
from ..params import build_params
from ..spaces import Box
from ._world_rollout import WorldRollout

_DF_ALIVE, _DF_DEAD, _DF_COLLISION, _DF_OOB, _DF_TEAM_WIN = 1, 16, 32, 64, 128  # dogfight.hpp, state group 6 word 3


class MAFixedwingDogfightEnv(WorldRollout):
    metadata = {"render_modes": [], "name": "ma_fixedwing_team_dogfight"}

    def __init__(self, team_size: int = 2, spawn_min_radius: float = 10.0, spawn_max_radius: float = 50.0,
                 spawn_min_height: float = 20.0, spawn_max_height: float = 50.0, damage_per_hit: float = 0.003,
                 lethal_distance: float = 20.0, lethal_angle_radians: float = 0.07, assisted_flight: bool = True,
                 aggressiveness: float = 0.5, cooperativeness: float = 0.5, sparse_reward: bool = False,
                 flatten_observation: bool = True, flight_dome_size: float = 800.0, max_duration_seconds: float = 60.0,
                 agent_hz: int = 30, render_mode=None, num_envs: int = 1, device="cuda:0", seed: int = 0, motor_noise: bool = True,
                 freeze_wrecks: bool = False):
        self._no_render(render_mode)
        self.assisted_flight = bool(assisted_flight)
        self.flatten_observation = bool(flatten_observation)
        self._check_agent_hz(agent_hz)
        if not 1 <= team_size <= 4:
            raise ValueError("team_size must be in 1..4 (the aircraft of a world share a wavefront: 2 * team_size <= 8)")
        # (spawn_min_height / spawn_max_height are accepted and unused, as in the reference: :197-201 draws the height
        #  between the RADIUS bounds)
        self.team_size = int(team_size)
        self._init_agents(2 * self.team_size, num_envs, device)
        self.team_flag = np.concatenate((np.zeros(self.team_size, dtype=bool), np.ones(self.team_size, dtype=bool)))
        self._df = dict(team_size=self.team_size, spawn_min_radius=spawn_min_radius, spawn_max_radius=spawn_max_radius,
                        damage_per_hit=damage_per_hit, lethal_distance=lethal_distance, lethal_angle=lethal_angle_radians,
                        aggressiveness=aggressiveness, cooperativeness=cooperativeness, sample_spawn=True, assisted_flight=self.assisted_flight,
                        freeze_wrecks=bool(freeze_wrecks))
        self._kw = dict(flight_dome_size=flight_dome_size, max_duration_seconds=max_duration_seconds, agent_hz=agent_hz,
                        sparse_reward=sparse_reward)
        self._noise = "philox" if motor_noise else "off"
        self._seed = int(seed)
        self._build(self._seed)
        ad = self.engine.action_dim  # 4, or 6 with assisted_flight=False (ma_fixedwing_base_env.py:69)
        self._action_space = Box(low=-np.ones(ad, dtype=np.float32), high=np.ones(ad, dtype=np.float32), dtype=np.float32)
        self._observation_space = Box(low=-np.inf, high=np.inf, shape=(self.engine.obs_dim,), dtype=np.float32)
        self.max_steps = self.engine.params.max_steps
        self.step_count = 0

    def _build(self, seed):
        # Aviary(world_scale=5.0, drone_type="fixedwing", drone_model="acrowing") (ma_fixedwing_base_env.py:193-210)
        P = build_params("fixedwing", "dogfight", noise=self._noise, autoreset="off", seed=seed, angle_representation="euler",
                         vehicle_options=dict(drone_model="acrowing"), world_options=dict(world_scale=5.0), dogfight=self._df, **self._kw)
        self.engine = BatchEngine(P, self.num_possible_agents * self.num_envs, device=self.device)

    def _obs_out(self, o):
        """The observation of one agent in the form `flatten_observation` asks for (pop_obs_by_id, :724-752)."""
        if self.flatten_observation:
            return o
        A, S = self.num_possible_agents, 19 + self.engine.action_dim  # self block: attitude 12, aux 6, health, past action
        if self.num_envs == 1:
            rows = o[S:].view(A - 1, 14)
            return {"self": o[:S], "others": rows[rows.abs().sum(dim=1) > 0]}  # active others only, in index order (:523-541)
        rows = o[:, S:].view(self.num_envs, A - 1, 14)
        return {"self": o[:, :S], "others": rows, "others_mask": rows.abs().sum(dim=2) > 0}

    @property
    def healths(self):
        """[num_envs, agents] float32 (self.healths of the reference)."""
        return self.engine.state[6, :, 0].view(self.num_envs, self.num_possible_agents)

    @property
    def start_pos(self):
        """[num_envs, agents, 3]: the spawn positions drawn at the last reset."""
        return self.engine.state[13, :, :3].view(self.num_envs, self.num_possible_agents, 3)

    # ------------------------------------------------------------------ ma_fixedwing_dogfight_env.py:215-322
    def reset(self, seed=None, options=None):
        if seed is not None:
            if int(seed) != self._seed:
                # current / past actions are created in __init__ and survive resets: groups 7-8, and 15 (entries 4, 5 of the
                # six-wide action space, assisted_flight=False)
                self._reseed(seed, keep=(slice(7, 9), 15))
            # a seeded reset replays the seed's stream from its start (np.random.RandomState(seed) in the reference, :187):
            # the counter RNG's event counters go back to zero; reset(seed=None) continues the stream
            self.engine.state[5, :, 2] = 0.0
            self._policy_step = 0
        self.step_count = 0
        self.agents = self.possible_agents[:]
        self.engine.env_reset()
        # the latch is the engine's (world_done, zeroed by the reset): step(), reset_envs() and rollout() / collect() keep ONE copy of it
        self._done = self.engine.world_done.view(torch.bool).view(self.num_envs, self.num_possible_agents)
        self._needs_reset = False
        obs = self._split(self.engine.obs)
        return {ag: self._obs_out(obs[i]) for i, ag in enumerate(self.possible_agents)}, {ag: dict() for ag in self.agents}

    def reset_envs(self, env_mask):
        """num_envs > 1: reset the copies selected by `env_mask` ([num_envs] bool) and leave the others running -- every agent
        of a selected copy starts a new episode (the reference's reset() of that env instance). Returns the observations of
        all copies (fresh ones for the selected copies)."""
        env_mask = torch.as_tensor(env_mask, dtype=torch.bool, device=self.device).view(self.num_envs)
        lane_mask = env_mask.repeat_interleave(self.num_possible_agents)
        self.engine.env_reset(mask=lane_mask)
        self._done[env_mask] = False
        self.agents = self.possible_agents[:]
        obs = self._split(self.engine.obs)
        return {ag: self._obs_out(obs[i]) for i, ag in enumerate(self.possible_agents)}

    @property
    def done(self):
        """[num_envs, agents] bool: latched per copy -- True from the step an agent's episode ended (termination or truncation)
        until that copy is reset. With num_envs > 1 the per-step `terminations` / `truncations` report the ending step only;
        this is what a caller culls by."""
        return self._done

    # ------------------------------------------------------------------ closed-loop rollouts (pz_envs/_world_rollout.py)
    _team1 = None  # [n] bool: the lanes of team 1 (agent index >= team_size), made when an opponent first flies them

    _pool_groups = None  # {P: [n] int32}: the segment index of every lane for a pool of P opponents

    def _world_args(self, opponent):
        if opponent is None:
            return None, None, None, 1
        if self._team1 is None:
            self._team1 = torch.as_tensor(self.team_flag, device=self.device).repeat(self.num_envs).contiguous()
        if not isinstance(opponent, (list, tuple)):
            return opponent, self._team1, None, 1
        P, A = len(opponent), self.num_possible_agents
        if not 1 <= P <= L.PF_OUTCOME_MAX_GROUPS or P > self.num_envs:
            raise ValueError(f"opponent: a pool holds 1..{L.PF_OUTCOME_MAX_GROUPS} policies and at most one per copy ({self.num_envs}), got {P}")
        if P == 1:
            return list(opponent), self._team1, None, 1
        groups = self._pool_groups = self._pool_groups or {}
        if P not in groups:
            # contiguous, near-equal segments of whole copies: dist.strong_shard's rule with unit = agents
            shards = [strong_shard(self.num_envs * A, p, P, unit=A) for p in range(P)]
            groups[P] = torch.repeat_interleave(torch.arange(P, dtype=torch.int32), torch.tensor([sh.lanes for sh in shards])).to(self.device)
        return list(opponent), self._team1, groups[P], P

    def _flat_infos(self):
        side = self.engine.state[6]
        bits = lambda: side[:, 3].view(torch.int32)
        return {"health": lambda: side[:, 0], "received_hits": lambda: side[:, 2].view(torch.int32), "dead": lambda: (bits() & _DF_DEAD) != 0,
                "collision": lambda: (bits() & _DF_COLLISION) != 0, "out_of_bounds": lambda: (bits() & _DF_OOB) != 0,
                "team_win": lambda: (bits() & _DF_TEAM_WIN) != 0}

    def rollout(self, policy, k_steps: int, opponent=None, store_mean: bool = False, outcomes: bool = False, pooled: bool = False):
        """`k_steps` closed-loop env steps of every copy, every action computed on the device by `policy` (a pyflyt_amd.MLPPolicy over
        the flattened observation) -- the loop of policy_act, step(), culling and reset_envs() without the host: a copy whose
        aircraft have ALL finished is reset on the device in the next step, which is no transition for any of them
        (BatchEngine.rollout_policy_worlds; four launches and one n-byte device copy per step, six and the copy with an opponent). Returns (obs [k, n, D], reward,
        terminated, truncated [k, n], actions [k, n, action width], valid [k, n] bool) and with store_mean the policy's means as a
        seventh: flat tensors with n = num_envs * agents, lane = copy * agents + agent -- t.view(k, num_envs, agents, ...) reads
        them per copy and aircraft. They belong to the engine and are overwritten by the next call with the same k_steps.
        `valid` is False where an aircraft sat the step out (finished before it: it flies on with zero commands, its reward and
        flags read 0), on the step that reset its copy, and on an opponent's lanes.
        `opponent`: a second MLPPolicy, frozen as far as this env is concerned, that flies team 1 (agent index >= team_size) from
        the same observations with the same noise keys; team 1's lanes are then never valid.
        The exploration noise's step index advances by k_steps per call and restarts with reset(seed=...). Afterwards `done` is
        the latch as the last step left it, `agents` the full list (as after reset_envs), and step() / reset_envs() go on from there.
        `opponent` may also be a list of 1 to 16 MLPPolicy, a pool (a league's past snapshots): the copies are cut into contiguous,
        near-equal segments of whole copies (dist.strong_shard's rule), segment p's team 1 is flown by entry p, and p is the lanes'
        group in outcome_counts. By default every entry costs one pf_policy_act over ALL rows and one merge onto its segment: P full
        launches and P merges per step, not P partial ones. opponent=[p] is opponent=p, bit for bit.
        pooled=True (with an opponent, one or a list; a ValueError without) takes the pool launch instead: the lanes are sorted by who
        flies them once per call (pf_policy_pool_plan) and every step's act is ONE pf_policy_act_pool for the learner and all its
        opponents, each row evaluated once by its own policy -- four launches per step whatever the pool's size. Every returned
        tensor, the final state and outcome_counts have the bits of pooled=False, with one difference: on an opponent's lanes, which
        are never valid, `mean` holds that opponent's own mean instead of the learner's.
        outcomes=True appends outcome [k, n] uint8 (pf_outcome_bit of every episode that ended: collision, out of bounds, team_win
        as PF_OC_COMPLETE, dead; team 1's lanes included) and outcome_counts [G, 16] int64 on the device, G = 1 or the pool's size:
        per group this call's episodes of the VALID lanes by cause (slots 0-9; slot 8 sums received_hits) and the copies that
        finished by result (10 worlds, 11 team 0 wins, 12 team 1 wins, 13 draws: a team won if one of its aircraft ended with
        team_win and none of the other team's did -- an opponent's lanes decide this although they are never valid). A copy is
        tallied in the step that resets it, so one that finishes in the call's last steps is counted by the next call; copies reset
        by reset() / reset_envs() are not tallied. One launch more per step. episode_outcomes_dict() reads a block back by name."""
        return self._world_rollout(policy, k_steps, opponent, store_mean, outcomes, pooled)

    def collect(self, policy, value_fn, k_steps: int, gamma: float = 0.99, lam: float = 0.95, opponent=None, stats: bool = False,
                normalize_reward: bool = False, outcomes: bool = False, pooled: bool = False):
        """One PPO batch from rollout()'s loop, as the vector envs' collect(): `value_fn` (a float32 [M, D] tensor -> [M] or [M, 1])
        runs under torch.no_grad() on all k + 1 observation rows, pf_gae (BatchEngine.gae) supplies advantages, returns and logp.
        Returns a dict with the vector envs' keys: obs [k, n, D] the policy's inputs, actions, mean, logp (None without a log_std),
        values, advantages, returns, valid, reward, terminated, truncated [k, n], last_value [n], infos (of the last step, lazy,
        over the flat lanes). Flat as in rollout(): t.view(k, num_envs, agents, ...). `valid` is rollout()'s (pf_world_sync's; pf_gae's
        own is all ones without an auto-reset mode): mask the losses with it -- pyflyt_amd.ppo_loss(env, ..., batch) does. A valid step's
        advantage depends on valid steps only: an episode's last step cuts the recursion, and a truncated aircraft bootstraps from
        its terminal observation, which the reset never overwrites (it lands in the row of the reset step).
        stats=True runs pf_traj_stats_masked (BatchEngine.traj_stats(valid=...)) on the same trajectory before pf_gae, with `valid` as
        the mask, and adds episode_return, episode_length [k, n] (the finished episode's return and length where an episode ended in
        a valid step, 0 elsewhere) and episode_summary ([8] float64 on the device; episode_summary_dict() reads it back); it updates
        the running moments behind obs_rms (the columns of the policy's inputs) and ret_rms (the discounted return, with this call's
        gamma) over the valid steps. normalize_reward=True implies stats, hands pf_gae reward / sqrt(ret_rms.var + 1e-8) with the
        moments AFTER this batch's update, and adds it as reward_scaled; reward stays raw. The steps a finished aircraft sits out and
        the step that resets its copy are in no return, length or moment, whatever their flags and rewards read. The per-lane
        carries need nothing extra: a copy is reset only after every one of its aircraft finished in a valid step, which zeroed
        that lane's carries; an opponent's lanes are never valid, so their carries stay zero and they are in no statistic. The
        episode accounting is carried from one collect(stats=True) to the next and sees only their steps: a step(), rollout() or
        collect() without stats in between advances the env behind its back, and the first episode_return / episode_length after
        it would lack those steps -- reset() the env before switching. reset() and reset_envs() zero the carries of the lanes they
        reset; reset(seed=other) keeps the running moments.
        `opponent` may be a pool, pooled=True flies it in the pool launch, and outcomes=True adds outcome and outcome_counts to the
        batch, all as rollout() describes them."""
        return self._world_collect(policy, value_fn, k_steps, gamma, lam, opponent, stats, normalize_reward, outcomes, pooled)

    # ------------------------------------------------------------------ ma_fixedwing_base_env.py:272-334
    def step(self, actions: dict):
        A, E = self.num_possible_agents, self.num_envs
        ad = self.engine.action_dim
        act = torch.zeros(E, A, ad, dtype=torch.float32, device=self.device)
        for k, v in actions.items():
            v = v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v), dtype=torch.float32)
            act[:, self.agent_name_mapping[k]] = v.to(self.device).view(E, ad)
        obs, rew, term, trunc = self.engine.env_step(act.view(E * A, ad))
        side = self.engine.state[6]
        o, r, t, u = self._split(obs), self._split(rew), self._split(term), self._split(trunc)
        health, hits, bits = self._split(side[:, 0]), self._split(side[:, 2].view(torch.int32)), self._split(side[:, 3].view(torch.int32))
        observations, rewards, terminations, truncations, infos = {}, {}, {}, {}, {}
        for ag in self.agents:
            i = self.agent_name_mapping[ag]
            observations[ag], rewards[ag], terminations[ag], truncations[ag] = self._obs_out(o[i]), r[i], t[i], u[i]
            infos[ag] = {"health": health[i], "received_hits": hits[i], "dead": (bits[i] & _DF_DEAD) != 0,
                         "collision": (bits[i] & _DF_COLLISION) != 0, "out_of_bounds": (bits[i] & _DF_OOB) != 0,
                         "team_win": (bits[i] & _DF_TEAM_WIN) != 0}
        self._done |= (term | trunc).view(E, A)
        self.step_count += 1
        # cull finished agents (:326-328); with num_envs > 1 an agent stays listed until it has finished in every copy (its
        # per-copy flags are in terminations / truncations; a copy's finished agent reports reward 0 from then on)
        alive = self._split((side[:, 3].view(torch.int32) & _DF_ALIVE) != 0)
        self.agents = [ag for ag in self.agents if bool(alive[self.agent_name_mapping[ag]].any())]
        return observations, rewards, terminations, truncations, infos
