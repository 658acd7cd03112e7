"""The contact rule of DESIGN section 24 in numpy and Python integers (which cannot overflow, so an int64 that would is
seen as a difference).  Restated from the rule, step by step in the order the section gives, not from the kernel: the
state is kept as the arrays `ContactMonitor.state()`, `pairs()` and `counts()` show, so a test compares them one for
one."""
import numpy as np

from tests.smooth_ref import wrap32

MAX_MM = (1 << 20) - 1
MEET, PART, LONG = 1, 2, 3
OUTPUTS = ('group', 'size', 'contacts', 'partner', 'together', 'events', 'n_events')
STATE = ('id', 'last', 'pos', 'frame', 'dropped')
PAIRS = ('link', 'since')
COUNTS = ('contacts', 'meets', 'parts', 'longs', 'groups', 'grouped', 'largest')


class ContactRef:
    def __init__(self, cameras=1, max_tracks=128, max_age=30, radius=1500, release=None, min_frames=3, long_frames=0,
                 max_events=256):
        self.cameras, self.S, self.max_age = cameras, max_tracks, max_age
        self.radius, self.release = radius, radius if release is None else release
        self.min_frames, self.long_frames, self.max_events = min_frames, long_frames, max_events
        C, S = cameras, max_tracks
        self.id = np.zeros((C, S), np.int32)
        self.last = np.zeros((C, S), np.int32)
        self.pos = np.zeros((C, S, 2), np.int32)
        self.link = np.zeros((C, S, S), np.int32)
        self.since = np.zeros((C, S, S), np.int32)
        self.frame = np.zeros(C, np.int32)
        self.dropped = np.zeros(C, np.int32)
        self.counters = {n: np.zeros(C, np.int32) for n in COUNTS}

    def reset(self, camera=None):
        c = slice(None) if camera is None else camera
        for a in (self.id, self.frame, self.dropped) + tuple(self.counters.values()):
            a[c] = 0

    def state(self, c):
        return {n: getattr(self, n)[c] for n in STATE}

    def pairs(self, c):
        return {n: getattr(self, n)[c] for n in PAIRS}

    def counts(self, c):
        return {n: self.counters[n][c] for n in COUNTS}

    def update(self, on, xy, ids, camera=0):
        """on [N], xy [N, 2], ids [N] -> dict of int32 group, size, contacts, partner, together [N], events
        [max_events, 7] and n_events (0-d)."""
        c, S = camera, self.S
        on, ids = np.asarray(on).reshape(-1), np.asarray(ids).reshape(-1)
        xy = np.clip(np.asarray(xy, np.int64).reshape(-1, 2), -MAX_MM, MAX_MM)
        N = len(on)
        self.frame[c] = wrap32(int(self.frame[c]) + 1)
        frame = int(self.frame[c])
        ident, link, since, count = self.id[c], self.link[c], self.since[c], self.counters
        events = []

        def add(name, by=1):
            count[name][c] = wrap32(int(count[name][c]) + by)

        def event(kind, s, t, frames, id_s, id_t, pose):
            a, b = (s, t) if id_s < id_t else (t, s)
            events.append((kind, min(id_s, id_t), max(id_s, id_t), wrap32(frames), pose.get(a, -1), pose.get(b, -1), frame))

        # 1, 2: the expiry and its PARTs, in ascending (s, t), before anybody is born
        held = ident.copy()
        gone = [t for t in range(S) if held[t] != 0 and frame - int(self.last[c, t]) > self.max_age]
        for s in range(S):
            for t in range(s + 1, S):
                if (s in gone or t in gone) and held[s] != 0 and held[t] != 0:
                    if link[s, t] & 1:
                        event(PART, s, t, frame - int(since[s, t]), int(held[s]), int(held[t]), {})
                        add('parts')
                    link[s, t] = since[s, t] = 0
        ident[gone] = 0
        # 1: who takes part, the slots and the births (a born slot's row and column are zeroed)
        slot, taken = [-1] * N, set()
        for d in range(N):
            if on[d] == 0 or int(ids[d]) < 1 or int(ids[d]) in taken:
                continue
            taken.add(int(ids[d]))
            have = np.nonzero(ident == ids[d])[0]
            slot[d] = int(have[0]) if len(have) else -2
        for d in range(N):
            if slot[d] == -2:
                free = np.nonzero(ident == 0)[0]
                if len(free):
                    t = slot[d] = int(free[0])
                    ident[t] = int(ids[d])
                    link[t, :] = link[:, t] = since[t, :] = since[:, t] = 0
                else:
                    slot[d] = -1
                    self.dropped[c] = wrap32(int(self.dropped[c]) + 1)
        pose = {}
        for d in range(N):
            if slot[d] >= 0:
                pose[slot[d]] = d
                self.pos[c, slot[d]], self.last[c, slot[d]] = xy[d], frame
        # 3, 4: the evaluation and the long contacts, in ascending (s, t)
        live = [t for t in range(S) if ident[t] != 0]
        for i, s in enumerate(live):
            for t in live[i + 1:]:
                contact, run = int(link[s, t]) & 1, int(link[s, t]) >> 8
                if s in pose and t in pose:
                    dx, dy = (int(v) for v in xy[pose[s]] - xy[pose[t]])
                    d2 = dx * dx + dy * dy
                    assert d2 < 1 << 44
                    near = int(d2 <= (self.release if contact else self.radius) ** 2)
                    if near == contact:
                        run = 0
                    else:
                        run += 1
                        if run >= self.min_frames:
                            run, contact = 0, 1 - contact
                            if contact:
                                since[s, t] = frame
                                event(MEET, s, t, 0, int(ident[s]), int(ident[t]), pose)
                                add('meets')
                            else:
                                event(PART, s, t, frame - int(since[s, t]), int(ident[s]), int(ident[t]), pose)
                                add('parts')
                                since[s, t] = 0
                    link[s, t] = contact | run << 8
                if contact and self.long_frames > 0 and wrap32(frame - int(since[s, t])) == self.long_frames:
                    event(LONG, s, t, self.long_frames, int(ident[s]), int(ident[t]), pose)
                    add('longs')
        # 5: the components of the live slots under the contact bits
        friends = {t: [u for u in live if u != t and link[min(t, u), max(t, u)] & 1] for t in live}
        party = {}
        for t in live:
            if t in party:
                continue
            members, todo = {t}, [t]
            while todo:
                for u in friends[todo.pop()]:
                    if u not in members:
                        members.add(u)
                        todo.append(u)
            for u in members:
                party[u] = members
        distinct = {id(m): m for m in party.values()}.values()
        count['contacts'][c] = sum(len(f) for f in friends.values()) // 2
        count['groups'][c] = sum(len(m) >= 2 for m in distinct)
        count['grouped'][c] = sum(len(m) for m in distinct if len(m) >= 2)
        count['largest'][c] = max([len(m) for m in distinct], default=0)
        # 6, 7: the outputs
        out = {n: np.zeros(N, np.int32) for n in OUTPUTS[:5]}
        for d in range(N):
            t = slot[d]
            if t < 0:
                continue
            out['group'][d] = min(int(ident[u]) for u in party[t])
            out['size'][d] = len(party[t])
            out['contacts'][d] = len(friends[t])
            if friends[t]:
                u = min(friends[t], key=lambda u: (int(since[min(t, u), max(t, u)]), u))
                out['partner'][d] = ident[u]
                out['together'][d] = wrap32(frame - int(since[min(t, u), max(t, u)]))
        table = np.zeros((self.max_events, 7), np.int32)
        stored = events[:self.max_events]
        if stored:
            table[:len(stored)] = np.asarray(stored, np.int64).astype(np.int32)
        out['events'], out['n_events'] = table, np.asarray(len(events), np.int32)
        return out
