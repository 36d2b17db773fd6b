"""A host model of the slot scheduler of the stream calls (csrc/runtime.hip: run_slot_queue), for the step counts the tests assert.

`done[i]` is the emitted step at which segment i's slowest group is done (a beam group: its W slots are full; it sets its rows' finished
flags in that step).  A segment admitted into a slot starts at position 0, feeds `n_prompt` prompt positions and then emits, so its flags
are all set once n_prompt + done[i] + 1 steps have run since its admission.  The host looks at the flags after every round of `interval`
steps, retires what has stopped and refills the freed slots from the queue, in slot order."""


def stream_steps(done, slots, interval, n_prompt=0):
    """steps launched by ymt3_transcribe_stream_beam (ymt3_last_decode_steps) for a queue of len(done) segments"""
    n = len(done)
    if n == 0:
        return 0
    interval = interval or 8
    slots = min(slots, n) if slots > 0 else n
    need = [n_prompt + int(d) + 1 for d in done]
    seg = list(range(slots))                    # the segment in every slot (None: empty)
    ran = [0] * slots                           # steps since its admission
    nxt, live, steps = slots, slots, 0
    while live:
        steps += interval
        free = []
        for s in range(slots):
            if seg[s] is None:
                continue
            ran[s] += interval
            if ran[s] >= need[seg[s]]:
                seg[s] = None
                live -= 1
                free.append(s)
        for s in free:
            if nxt < n:
                seg[s], ran[s] = nxt, 0
                nxt += 1
                live += 1
    return steps


def lockstep_steps(done, bsz, interval, n_prompt, n_steps):
    """steps launched by lock-step beam calls on batches of `bsz` segments with ymt3_set_early_stop(interval): a batch feeds its prompt,
    then runs chunks of `interval` steps until a check finds every group done (or n_steps have run)"""
    total = 0
    for i in range(0, len(done), bsz):
        last = max(int(d) for d in done[i:i + bsz]) + 1
        total += n_prompt + min(n_steps, interval * -(-last // interval))
    return total
