"""A small exhaustive model of the exchange-ring protocol of the fp32 GRU team kernels (gru_dev.h "exchange ring"): host only.

The model: 3 workgroups, each producer of one slice of every slot and consumer of all three, 2 waves each.  The waves of a workgroup split the
operand as the K-split waves of a team do: wave 0 (a gate wave: it stores the workgroup's value) reads the slices of producers 0 and 1, wave 1
(the re-arming wave) that of producer 2.  In iteration q a wave
    reads   its producers' slices of slot (q - 1) % R (q > 0) -- data is the flag: a read completes on anything but the sentinel, and the value it
            takes must be q - 1;
    meets   its partner at the team barrier of q;
    stores  behind it: wave 0 the value q into its workgroup's slice of slot q % R, wave 1 the sentinel over the slice of the slot that held
            iteration q - 2 (R = 4: slot (q + 2) % 4), unless q < 2 (the launcher armed that slot) or iteration q + 2 does not exist.
Memory: a store is issued into the wave's own set of pending stores and becomes visible at ANY later moment, in any order with every other
pending store of any wave -- except that a wave's loads return behind its own earlier stores (vmcnt counts both and retires in issue order), so
a wave completes no read while a store of its own is pending.  An acknowledged wait plus the team barrier is thus the only ordering between the
stores of two waves, as in the kernels.  Every interleaving of the six waves and of the moments stores become visible is enumerated (a
breadth-first walk over the reachable states) for 6 iterations: the first re-armed slot is slot 0 in iteration 2, it takes data in iteration 4
and is read in iteration 5.

Two things can go wrong, and the walk reports the first it meets: a reader takes a value of another iteration ('stale'), or a value is
destroyed before every reader has it and its readers wait for ever ('starved': the kernels would run into their 2 s spin bound).

So that the argument has teeth: 3 slots, or the re-arm placed in front of the team barrier (where the re-arming wave knows only that ITS
producers are past iteration q - 1, not its partner's), must both be caught."""
from collections import deque

SENT = -1
WG, WAVES, ITERS = 3, 2, 6
READS = ((0, 1), (2,))          # producers whose slices wave 0 / wave 1 of every workgroup reads


def explore(R, rearm_after_barrier=True, iters=ITERS):
    """-> (verdict, states): verdict None (no interleaving goes wrong), or ('stale' | 'starved', a description)"""
    # a wave's place: (q, pc), pc = 0 .. len(reads) - 1: next read; len(reads): in front of the barrier; len(reads) + 1: arrived (waiting
    # for the partner); the stores are issued in the step that leaves the barrier
    def slot_of(q):
        return q % R

    nwaves = WG * WAVES
    mem0 = tuple(SENT for _ in range(WG * R))                     # mem[w * R + slot]: the launcher's fill
    start = (tuple((0, len(READS[k % WAVES])) for k in range(nwaves)),      # iteration 0 reads nothing
             tuple(() for _ in range(nwaves)), mem0)
    seen = {start}
    todo = deque([start])
    while todo:
        st = todo.popleft()
        place, pend, mem = st
        nxt = []
        for k in range(nwaves):
            w, v = divmod(k, WAVES)
            q, pc = place[k]
            if q >= iters:
                continue
            # a pending store of this wave becomes visible
            for i, (cell, val) in enumerate(pend[k]):
                m2 = mem[:cell] + (val,) + mem[cell + 1:]
                p2 = pend[:k] + (pend[k][:i] + pend[k][i + 1:],) + pend[k + 1:]
                nxt.append((place, p2, m2))
            rd = READS[v]
            if pc < len(rd):                                      # a read: behind this wave's own stores, and only of something written
                if pend[k]:
                    continue
                got = mem[rd[pc] * R + slot_of(q - 1)]
                if got == SENT:
                    continue
                if got != q - 1:
                    return ('stale', 'workgroup %d wave %d, iteration %d, takes the value of iteration %d from producer %d (slot %d)'
                            % (w, v, q, got, rd[pc], slot_of(q - 1))), len(seen)
                nxt.append((place[:k] + ((q, pc + 1),) + place[k + 1:], pend, mem))
                continue
            rearm = v == 1 and q >= 2 and q + 2 < iters
            if pc == len(rd):                                     # arrive at the barrier (the misplaced re-arm is issued in front of it)
                p2 = pend
                if rearm and not rearm_after_barrier:
                    p2 = pend[:k] + (pend[k] + ((w * R + slot_of(q - 2), SENT),),) + pend[k + 1:]
                nxt.append((place[:k] + ((q, pc + 1),) + place[k + 1:], p2, mem))
                continue
            # at the barrier: leave once the partner has arrived (or is already past it), issuing this wave's stores
            pq, ppc = place[w * WAVES + (1 - v)]
            if pq > q or (pq == q and ppc == len(READS[1 - v]) + 1):
                add = ()
                if v == 0:
                    add = ((w * R + slot_of(q), q),)
                elif rearm and rearm_after_barrier:
                    add = ((w * R + slot_of(q - 2), SENT),)
                nq = q + 1
                p2 = pend[:k] + (pend[k] + add,) + pend[k + 1:]
                nxt.append((place[:k] + ((nq, 0),) + place[k + 1:], p2, mem))
        if not nxt and any(q < iters for q, _ in place):
            stuck = [(k // WAVES, k % WAVES, place[k][0]) for k in range(nwaves) if place[k][0] < iters and place[k][1] < len(READS[k % WAVES])]
            return ('starved', 'no wave can move; waiting readers (workgroup, wave, iteration): %s' % stuck), len(seen)
        for s in nxt:
            if s not in seen:
                seen.add(s)
                todo.append(s)
    return None, len(seen)


def test_four_slots_rearm_behind_the_barrier_is_safe():
    verdict, states = explore(4, True)
    assert verdict is None, verdict
    assert states > 10000          # (the walk really went through the interleavings)


def test_three_slots_give_a_stale_read():
    """the slot would take data one iteration after the re-arm, and a consumer polls it having seen nothing that is ordered behind the re-arm"""
    verdict, _ = explore(3, True)
    assert verdict is not None and verdict[0] == 'stale', verdict


def test_rearm_in_front_of_the_barrier_is_caught():
    """the re-arming wave has seen iteration q - 1 of ITS producers only: a consumer among its partner's producers may still be reading the slot"""
    verdict, _ = explore(4, False)
    assert verdict is not None, 'the misplaced re-arm went unnoticed'
