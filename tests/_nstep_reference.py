"""A numpy model of the device replay ring under the pool's loop, for the n-step tests (gvec_nstep_link / gvec_nstep_gather;
DESIGN.md 4.11).  Every row it pushes carries an explicit (worker, episode, t) tag, so n-step chains can be found by brute
force over the tags - never looking at a link - and compared with the walk over the links the model keeps the way the
device does.  The observation's first float carries the same tag, so a test can also check a batch with no model at all."""
import numpy as np

TAG_T, TAG_E = 32, 64                      # tag = (worker * TAG_E + episode) * TAG_T + t: exact in float32 below 2^24


def tag_of(worker, episode, t):
    return (worker * TAG_E + episode) * TAG_T + t


def untag(tag):
    tag = np.asarray(tag).astype(np.int64)
    return tag // (TAG_E * TAG_T), tag // TAG_T % TAG_E, tag % TAG_T


def script(num_envs, steps, max_steps_per_episode, obs_floats, seed=1, p_done=0.1):
    """The per-step tensors a pool would hand gvec_pool_collect, generated as the pool generates them: at step 0 every worker
    is in its reset, was_reset[t + 1] = over[t], done drawn with p = 0.1, over = live & (done | length >= limit).
    state[w][0] is the tag of the worker's (episode, t), next_state[w][0] the tag of t + 1."""
    assert num_envs * TAG_E * TAG_T < 1 << 24 and max_steps_per_episode < TAG_T
    rng = np.random.default_rng(seed)
    fill = np.random.default_rng(seed + 1000)
    was_reset = np.ones(num_envs, bool)
    length = np.zeros(num_envs, np.int64)
    episode = np.zeros(num_envs, np.int64)
    out = []
    for _ in range(steps):
        done = rng.random(num_envs) < p_done
        live = ~was_reset
        state = fill.standard_normal((num_envs, obs_floats)).astype(np.float32)
        nxt = fill.standard_normal((num_envs, obs_floats)).astype(np.float32)
        w = np.arange(num_envs)
        state[:, 0] = tag_of(w, episode, length)
        nxt[:, 0] = tag_of(w, episode, length + 1)
        coin = fill.random(num_envs) < 0.5
        step = dict(state=state, next_state=nxt, action=fill.integers(0, 1000, num_envs).astype(np.int64),
                    reward=fill.standard_normal(num_envs).astype(np.float64), terminated=(done & coin).astype(np.uint8),
                    truncated=(done & ~coin).astype(np.uint8), was_reset=was_reset.astype(np.uint8))
        length = length + live
        over = live & (done | (length >= max_steps_per_episode))
        assert int(episode.max()) + 1 < TAG_E
        length[over] = 0
        episode[over] += 1
        was_reset = over
        out.append(step)
    return out


class RingModel:
    def __init__(self, num_envs, capacity, max_steps_per_episode, obs_floats):
        self.n, self.cap, self.limit = num_envs, capacity, max_steps_per_episode
        self.state = np.zeros((capacity, obs_floats), np.float32)
        self.next_state = np.zeros((capacity, obs_floats), np.float32)
        self.action = np.zeros(capacity, np.int64)
        self.reward = np.zeros(capacity, np.float64)
        self.done = np.zeros(capacity, bool)
        # the tags: who wrote the row, and whether the worker's episode ended with it (done, or cut at the limit)
        self.worker = np.full(capacity, -1, np.int64)
        self.episode = np.full(capacity, -1, np.int64)
        self.t = np.full(capacity, -1, np.int64)
        self.seq = np.full(capacity, -1, np.int64)
        self.ended = np.zeros(capacity, bool)
        self.cursor = self.size = self.total = 0
        # what the device keeps
        self.succ = np.full(capacity, -1, np.int64)
        self.last = np.full((num_envs, 2), -1, np.int64)
        self.length = np.zeros(num_envs, np.int64)
        self.ep = np.zeros(num_envs, np.int64)
        self.skipped_links = self.links = self.ended_by_done = self.ended_by_cut = 0

    def step(self, x):
        live = ~x["was_reset"].astype(bool)
        done = (x["terminated"] | x["truncated"]).astype(bool)
        self.length[live] += 1
        over = live & (done | (self.length >= self.limit))
        new = []
        for w in np.flatnonzero(live):
            s, q = self.cursor, self.total
            self.state[s], self.next_state[s] = x["state"][w], x["next_state"][w]
            self.action[s], self.reward[s], self.done[s] = x["action"][w], x["reward"][w], done[w]
            self.worker[s], self.episode[s], self.t[s], self.seq[s], self.ended[s] = w, self.ep[w], self.length[w] - 1, q, over[w]
            self.cursor = (s + 1) % self.cap
            self.size = min(self.size + 1, self.cap)
            self.total += 1
            new.append((w, q, s))
        for w, q, s in new:
            pq, ps = self.last[w]
            if pq >= 0:
                if pq >= self.total - self.cap:       # still held, by arithmetic alone
                    self.succ[ps] = s
                    self.links += 1
                else:
                    self.skipped_links += 1
            self.succ[s] = -1
            self.last[w] = (-1, -1) if over[w] else (q, s)
        self.ended_by_done += int((over & done).sum())
        self.ended_by_cut += int((over & ~done).sum())
        self.length[over] = 0
        self.ep[over] += 1

    # ---- the two walks ------------------------------------------------------------------------------------------
    def _by_tag(self):
        return {(int(self.worker[s]), int(self.episode[s]), int(self.t[s])): s for s in range(self.size) if self.worker[s] >= 0}

    def _fold(self, chain, gamma):
        """(ret, discount) of a chain of slots: every float64 operation in the order the header gives."""
        gamma = np.float64(gamma)
        ret, disc = np.float64(self.reward[chain[0]]), np.float64(1.0)
        for s in chain[1:]:
            disc = disc * gamma
            ret = ret + disc * np.float64(self.reward[s])
        return ret, disc * gamma

    def chain_by_tags(self, i, n_step, by_tag=None):
        """Slots of the chain that starts at held slot i, found from the tags alone."""
        by_tag = self._by_tag() if by_tag is None else by_tag
        chain = [i]
        while len(chain) < n_step:
            c = chain[-1]
            if self.done[c] or self.ended[c] or self.worker[c] < 0:
                break
            nx = by_tag.get((int(self.worker[c]), int(self.episode[c]), int(self.t[c]) + 1))
            if nx is None:
                break
            chain.append(nx)
        return chain

    def chain_by_links(self, i, n_step):
        chain = [i]
        while len(chain) < n_step and not self.done[chain[-1]] and self.succ[chain[-1]] >= 0:
            chain.append(int(self.succ[chain[-1]]))
        return chain

    def gather(self, idx, n_step, gamma, by="links"):
        """What gvec_nstep_gather returns for idx: a dict of arrays."""
        k, F = len(idx), self.state.shape[1]
        o = dict(state=np.zeros((k, F), np.float32), next_state=np.zeros((k, F), np.float32), action=np.full(k, -1, np.int64),
                 ret=np.zeros(k), discount=np.zeros(k), done=np.zeros(k, bool), steps=np.zeros(k, np.int32), last_idx=np.full(k, -1, np.int64))
        by_tag = self._by_tag() if by == "tags" else None
        for j, i in enumerate(idx):
            i = int(i)
            if i < 0 or i >= self.size:
                continue
            chain = self.chain_by_links(i, n_step) if by == "links" else self.chain_by_tags(i, n_step, by_tag)
            c = chain[-1]
            o["state"][j], o["next_state"][j], o["action"][j] = self.state[i], self.next_state[c], self.action[i]
            o["ret"][j], o["discount"][j] = self._fold(chain, gamma)
            o["done"][j], o["steps"][j], o["last_idx"][j] = self.done[c], len(chain), c
        return o

    def full_chain_fraction(self, n_step):
        by_tag = self._by_tag()
        return float(np.mean([len(self.chain_by_tags(i, n_step, by_tag)) == n_step for i in range(self.size)]))


def run(num_envs, capacity, steps, max_steps_per_episode, obs_floats, seed=1):
    """(script, model after the last step)."""
    sc = script(num_envs, steps, max_steps_per_episode, obs_floats, seed)
    m = RingModel(num_envs, capacity, max_steps_per_episode, obs_floats)
    for x in sc:
        m.step(x)
    return sc, m
