"""Batched image+prompt serving on one replica, and the data-parallel wrapper around it (BASELINE.json configs[3]: 32 requests over 8 GPUs).

A request = (image, prompt) owns its embedding, KV cache and position, so a replica can run several of them side by side:

  * the images of a wave are encoded in ONE pass over the vision weights (`minigpt4_amd_encode_images`, up to 8 per pass);
  * every request gets its own conversation of the context (`minigpt4_amd_set_conversations` / `_select_conversation`) and is prompted through the
    reference entry points exactly as `MiniGPT4ChatBot.generate` does (`minigpt4_library.py:627-644` of the reference): system prompt, image turn;
  * decode steps run for all unfinished conversations at once (`minigpt4_amd_end_chat_batch`: one pass over the LLM weights per 4 conversations);
  * per conversation the reference's stop rule applies: a piece equal to "##" is swallowed, the answer ends when the accumulated text ends with "###"
    (`minigpt4_contains_eos_token` / `minigpt4_is_eos`, reference `generate`), or after `max_tokens`.

Sessions: a conversation can outlive its wave.  `suspend(slot)` takes a conversation out of its slot as one checksummed blob (`minigpt4_amd_state_save`) and
`resume(slot, blob)` puts it into any slot (`minigpt4_amd_state_load`); `run(..., sessions=[...])` uses the pair to serve follow-up turns of more sessions than there
are slots: after a wave every request that names a session is parked, and a later request of that session (image None) is resumed and asked with
`minigpt4_begin_chat` instead of paying the image turn and all earlier turns again.

Across GPUs requests shard round-robin (`dist.shard_requests`); ranks exchange nothing per token and the answers are gathered at the end.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np

from . import dist as D
from . import minigpt4_library as ML


@dataclass
class Request:
    image: Union[str, bytes, np.ndarray, None]   # file path, encoded image bytes (PNG / JPEG / ...), or a preprocessed f32 [3][224][224] array; None: a follow-up turn of a session
    prompt: str
    max_tokens: int = 64


def plan_waves(n_requests: int, conversations: int) -> List[List[int]]:
    """Requests are served in waves of `conversations`; inside a wave they decode together until each one stops."""
    return [list(range(i, min(n_requests, i + conversations))) for i in range(0, n_requests, conversations)]


def ngram_draft(history: Sequence[int], ngram_max: int = 3, ngram_min: int = 1, n_draft: int = 4) -> List[int]:
    """The n-gram drafter of lookup decoding (csrc/draft.hpp, `minigpt4_amd_decode_lookup`), in Python for the serving loop: the longest suffix of `history`
    (ngram_max down to ngram_min tokens, ending in its last token) that also starts at an earlier index, its most recent occurrence; the tokens that followed it, cut at
    n_draft, before the first id 2 (</s>) and at the end of the history.  [] = no match."""
    if ngram_min < 1 or ngram_max < ngram_min or n_draft < 0:
        raise ValueError("ngram_draft: need 1 <= ngram_min <= ngram_max and n_draft >= 0")
    h = [int(t) for t in history]
    n = len(h)
    if n_draft < 1:
        return []
    for length in range(min(ngram_max, n - 1), ngram_min - 1, -1):
        tail = h[n - length:]
        for s in range(n - length - 1, -1, -1):
            if h[s:s + length] == tail:
                out = []
                for t in h[s + length:]:
                    if len(out) >= n_draft or t == 2:
                        break
                    out.append(t)
                return out
    return []


class ReplicaServer:
    def __init__(self, vision_path: str, llm_path: str, conversations: int = 4, n_ctx: int = 2048, n_batch: int = 512, seed: int = 1337,
                 library: Optional[ML.MiniGPT4SharedLibrary] = None, verbosity: int = 0, rank: int = 0, world: int = 1, device=None, prefix_cache: int = 0):
        """world > 1 (inside an initialised `torch.distributed` job): the replica is loaded through `dist.load_replica` -- rank 0 reads the files, every other
        rank loads headers only and receives both weight arenas by broadcast, so the weights cross the file system once per node.
        prefix_cache > 0: the engine's prefix cache with that many rows (`minigpt4_amd_set_prefix_cache`): the constant head of every request (system prompt +
        "Human: <Img>") is evaluated by the first request and copied by the others, in the per-conversation and in the batched prefill alike."""
        self.lib = library or ML.load_library()
        self.load_stats = None
        if world > 1:
            self.ctx, self.load_stats = D.load_replica(self.lib, vision_path, llm_path, rank, world, device=device, verbosity=verbosity, seed=seed, n_ctx=n_ctx, n_batch=n_batch)
        else:
            self.ctx = self.lib.minigpt4_model_load(vision_path, llm_path, verbosity=verbosity, seed=seed, n_ctx=n_ctx, n_batch=n_batch)
        self.conversations = conversations
        self.lib.amd_set_conversations(self.ctx, conversations)
        if prefix_cache:
            self.lib.amd_set_prefix_cache(self.ctx, prefix_cache)
        self._parked = {}                      # session id -> snapshot of the idle session
        self._speculation = False              # run(lookup=...) switches draft verification on at its first use
        self._row_cap = min(64, max(n_batch, 32, conversations))   # rows one verify pass holds: 64, and the context's activation rows (include/minigpt4_amd.h)

    def suspend(self, slot: int) -> bytes:
        """Conversation `slot` as a snapshot (queued rows are evaluated first); the slot is reset and free for another conversation."""
        blob = self.lib.amd_state_save(self.ctx, slot)
        self.lib.amd_select_conversation(self.ctx, slot)
        self.lib.minigpt4_reset_chat(self.ctx)
        return blob

    def resume(self, slot: int, blob: bytes) -> None:
        """Put a suspended conversation into `slot` (whatever it held is dropped): it continues bit for bit where `suspend` took it."""
        self.lib.amd_state_load(self.ctx, slot, blob)

    def parked_sessions(self) -> List:
        return list(self._parked)

    def drop_session(self, session) -> None:
        self._parked.pop(session, None)

    def close(self):
        if self.ctx is not None:
            self.lib.minigpt4_free(self.ctx)
            self.ctx = None

    # ---- image -> MiniGPT4Image (F32 CHW), through the library's own loader / preprocess kernels for files and bytes
    def _to_struct(self, image):
        if isinstance(image, np.ndarray):
            return ML.array_to_image_struct(image), []
        raw = self.lib.amd_decode_image(image) if isinstance(image, (bytes, bytearray)) else self.lib.minigpt4_image_load_from_file(self.ctx, image)
        pre = self.lib.minigpt4_preprocess_image(self.ctx, raw)
        return pre, [raw, pre]

    def run(self, requests: Sequence[Request], temp: float = 0.0, top_k: int = 40, top_p: float = 0.9, ignore_eos: bool = False,
            batched_prefill: bool = False, logprobs: int = 0, repeat_penalty: float = 1.0, repeat_last_n: int = 64, presence_penalty: float = 0.0,
            frequency_penalty: float = 0.0, logit_bias=None, num_beams: int = 1, length_penalty: float = 1.0, guidance_scale: float = 1.0,
            negative_prompt: Optional[str] = None, regex=None, sessions: Optional[Sequence] = None, device_sampling: bool = False,
            seeds: Optional[Sequence[int]] = None, tfs_z: float = 1.0, typical_p: float = 1.0, min_p: float = 0.0, mirostat: int = 0, mirostat_tau: float = 5.0,
            mirostat_eta: float = 0.1, lookup: int = 0) -> List[str]:
        """lookup = n_draft (1 .. 7; 0, the default, is exactly the decode loop below): greedy lookup decoding for the whole wave.  Every iteration of the decode loop is
        ONE `minigpt4_amd_verify_draft_batch`: each unfinished request brings its next token and up to n_draft guesses behind it -- `ngram_draft` over the request's
        tokenized prompt followed by the tokens it has emitted, cut at the tokens the request still wants -- through one weight pass and keeps the guesses the pass's own
        logits confirm, so the answers are those of temp = 0 without lookup.  The kept tokens go through the same piece-by-piece stop rule; tokens kept behind the stop are
        discarded.  A pass holds 64 rows (and no more than the context's activation rows, max(n_batch, 32, conversations)): drafts are shortened, in slot order,
        where the wave's rows would not fit.  (A request's first iteration sends no guess: the pass itself tells which token comes next.)  One difference from the plain loop: on a full context
        that cannot shift the request ENDS (the pass leaves it out), where the plain loop goes on emitting the token it cannot evaluate until max_tokens.  `minigpt4_amd_set_speculation(7)` is called at first
        use.  The pass decides on raw logits at temp <= 0 only, so ValueError together with temp > 0, penalties, logit_bias, regex, logprobs, num_beams > 1,
        guidance_scale != 1, device_sampling, and sessions (a parked snapshot would hold rows behind the stop).
        tfs_z, typical_p, min_p, mirostat (0 or 2), mirostat_tau, mirostat_eta: the extended rule of device-side sampling (include/minigpt4_amd.h), honoured with
        device_sampling=True -- every step is then ONE `minigpt4_amd_end_chat_batch_sampled_ex`, and a request's mirostat mu is its own: unset
        (`minigpt4_amd_conversation_mirostat`) when the request takes its slot, so its text does not depend on its partners.  A non-neutral value without
        device_sampling raises ValueError (the host chain's mirostat state is the context's).
        device_sampling (the decode loop only, temp > 0): every step is ONE `minigpt4_amd_end_chat_batch_sampled` -- the tokens are sampled on the device (top-k <= 64,
        top-p, temperature; include/minigpt4_amd.h states the rule) and handed to the weight pass without a host visit, and every request draws from a stream of its own:
        seeds (one 64-bit integer per request; None: the request's index) is set with `minigpt4_amd_conversation_seed(slot, seed, 0)` when the request takes its slot, so
        a request's text does not depend on which other requests share its wave or on its slot.  Works with regex, penalties and logit_bias; ValueError together with
        num_beams > 1, guidance_scale != 1 or logprobs > 0, with temp <= 0, and for seeds without device_sampling or of another length than requests.
        sessions (one hashable id or None per request; the decode loop only -- ValueError with num_beams > 1 or guidance_scale != 1): a request that names a session is
        parked when its wave ends (`suspend`), so the server holds any number of idle sessions next to its `conversations` slots.  A request whose session is parked
        is a FOLLOW-UP turn: its image must be None, the session is resumed into the wave's slot and the prompt asked with `minigpt4_begin_chat`; the image turn and
        every earlier turn are not evaluated again.  A session may appear once per call.  `drop_session` forgets one.
        regex (str or bytes; include/minigpt4_amd.h states the pattern language): constrained decoding -- the pattern is compiled once for the call
        (`minigpt4_amd_constraint_compile`), set on every request's conversation and cleared and freed when the call returns; every answer then matches the WHOLE pattern, or is
        a prefix of a match when max_tokens ran out first.  The answer ends at "</s>", which the constraint allows exactly where the text matches; the "###" / "##" rules
        of the decode loop are off (the pattern decides what the text may hold).  Works with temp > 0, logprobs, penalties and logit_bias; ValueError together with
        num_beams > 1 or guidance_scale != 1 (those paths decide on their own rows).
        guidance_scale != 1: guided decoding (classifier-free guidance, `minigpt4_amd_end_chat_guided`) -- every request takes two conversations, so a wave holds
        conversations // 2 requests: its own, and a guidance conversation that gets the system prompt and `minigpt4_begin_chat` of the request's prompt WITHOUT the image
        (negative_prompt given: of that text instead); with batched_prefill both kinds go into the one `minigpt4_amd_prefill_batch`.  Every step decides one token per
        request from the two conversations' logits (scale > 1 pushes away from the guidance conversation) and advances both; penalties and logit bias act on the guided
        row, the stop rule is the decode loop's.  Not available with logprobs > 0 or num_beams > 1.  guidance_scale = 1 (the default) is exactly the decode loop below.
        num_beams > 1: beam search (`minigpt4_amd_beam_search`) instead of the decode loop -- every request takes num_beams conversations (its own and num_beams - 1 of
        scratch), so a wave holds conversations // num_beams requests; the answer is the best hypothesis (final score = sum of log-probabilities / length ** length_penalty),
        cut by the same "###" rule.  The search decides on raw logits: temp / top_k / top_p, penalties and logit bias do not enter it; logprobs is not available with it.
        num_beams = 1 (the default) is exactly the decode loop below.
        repeat_penalty / repeat_last_n / presence_penalty / frequency_penalty / logit_bias ({id: bias} or (id, bias) pairs): llama.cpp's penalties and a logit
        bias for every request of the call (include/minigpt4_amd.h), applied per conversation before the decode loop and taken back when the call returns.  The
        defaults are neutral: the call then touches none of it.
        logprobs > 0: the decode loop uses `minigpt4_amd_end_chat_batch_top` (same pieces, same sampler draws) and `self.last_logprobs[i]` holds, per generated
        token of request i (swallowed "##" pieces included), dict(id, piece, logprob, rank, top=[(piece, logprob), ...]) with `logprobs` alternatives -- the
        log-probabilities of the raw logits, whatever temp / top_k / top_p.  The return value is the same."""
        lib, ctx = self.lib, self.ctx
        if lookup:
            if isinstance(lookup, bool) or not isinstance(lookup, int) or not 1 <= lookup <= 7:
                raise ValueError("lookup must be 0 (off) or 1 .. 7 draft tokens")
            bad = [name for name, on in (("temp > 0", temp > 0), ("penalties", repeat_penalty != 1.0 or presence_penalty != 0.0 or frequency_penalty != 0.0),
                                         ("logit_bias", bool(logit_bias)), ("regex", regex is not None), ("logprobs", logprobs > 0), ("num_beams > 1", num_beams > 1),
                                         ("guidance_scale != 1", guidance_scale != 1.0), ("device_sampling", bool(device_sampling)), ("sessions", sessions is not None)) if on]
            if bad:
                raise ValueError("lookup decides greedily on raw logits: not available with " + ", ".join(bad))
        if num_beams < 1 or num_beams > 8 or num_beams > self.conversations:
            raise ValueError("num_beams must be 1 .. min(8, conversations)")
        if num_beams > 1 and logprobs > 0:
            raise ValueError("logprobs is not available with num_beams > 1")
        guided = guidance_scale != 1.0
        if guided and not np.isfinite(guidance_scale):
            raise ValueError("guidance_scale must be finite")
        if guided and (logprobs > 0 or num_beams > 1):
            raise ValueError("guidance_scale != 1 is not available with logprobs > 0 or num_beams > 1")
        if guided and self.conversations < 2:
            raise ValueError("guidance_scale != 1 takes two conversations per request")
        if regex is not None and (num_beams > 1 or guided):
            raise ValueError("regex is not available with num_beams > 1 or guidance_scale != 1")
        if device_sampling:
            if num_beams > 1 or guided or logprobs > 0:
                raise ValueError("device_sampling is not available with num_beams > 1, guidance_scale != 1 or logprobs > 0")
            if not (np.isfinite(temp) and temp > 0):
                raise ValueError("device_sampling needs temp > 0")
            if top_k < 1 or top_k > 64 or not (0 < top_p <= 1):
                raise ValueError("device_sampling needs top_k in 1 .. 64 and top_p in (0, 1]")
            if seeds is not None and len(seeds) != len(requests):
                raise ValueError("seeds: one integer per request")
            seeds = [int(s_) & 0xFFFFFFFFFFFFFFFF for s_ in (range(len(requests)) if seeds is None else seeds)]
        elif seeds is not None:
            raise ValueError("seeds needs device_sampling=True")
        chain = dict(tfs_z=tfs_z, typical_p=typical_p, min_p=min_p, mirostat=mirostat, mirostat_tau=mirostat_tau, mirostat_eta=mirostat_eta)
        extended = lib._chain_args("device_sampling", **chain)               # ValueError "device_sampling: ..." for a value out of range
        if extended and not device_sampling:
            raise ValueError("tfs_z, typical_p, min_p and mirostat need device_sampling=True")
        chain = chain if extended else None
        if sessions is not None:
            if num_beams > 1 or guided:
                raise ValueError("sessions is not available with num_beams > 1 or guidance_scale != 1")
            named = [s_ for s_ in sessions if s_ is not None]
            if len(sessions) != len(requests) or len(set(named)) != len(named):
                raise ValueError("sessions: one id (or None) per request, each session at most once per call")
            for r, s_ in zip(requests, sessions):
                if (r.image is None) != (s_ is not None and s_ in self._parked):
                    raise ValueError("sessions: a request without an image must name a parked session, a request with one must not")
        elif any(r.image is None for r in requests):
            raise ValueError("a request without an image needs sessions=")
        answers: List[str] = [""] * len(requests)
        self._constraint = lib.amd_constraint_compile(ctx, regex) if regex is not None else 0   # a refused pattern raises before anything is touched
        penalised = repeat_penalty != 1.0 or presence_penalty != 0.0 or frequency_penalty != 0.0
        mode_before = lib.amd_penalty_info(ctx)["mode"] if penalised else 0
        try:
            return self._run(requests, answers, temp, top_k, top_p, ignore_eos, batched_prefill, logprobs, penalised, logit_bias,
                             dict(repeat_last_n=repeat_last_n, repeat_penalty=repeat_penalty, alpha_presence=presence_penalty, alpha_frequency=frequency_penalty),
                             num_beams, length_penalty, guidance_scale if guided else None, negative_prompt, sessions, seeds if device_sampling else None, chain, lookup)
        finally:
            if self._constraint:
                for slot in range(self.conversations):
                    lib.amd_set_constraint(ctx, slot, 0)
                lib.amd_constraint_free(ctx, self._constraint)
                self._constraint = 0
            if penalised or logit_bias:
                for slot in range(self.conversations):
                    lib.amd_select_conversation(ctx, slot)
                    lib.amd_conversation_penalties(ctx, slot)
                    lib.amd_set_logit_bias(ctx, None)
                lib.amd_select_conversation(ctx, 0)
            if penalised:
                lib.amd_set_penalties(ctx, bool(mode_before))

    def _beam_answer(self, slots, max_tokens, length_penalty, ignore_eos) -> str:
        """The best hypothesis of a beam search from conversation slots[0], as the decode loop would have shown its pieces."""
        lib, ctx = self.lib, self.ctx
        if max_tokens <= 0:
            return ""
        ids, _ = lib.amd_beam_search(ctx, slots, max_tokens, length_penalty, n_best=1)[0]
        text = shown = ""
        for t in ids:
            if int(t) == 2:                                       # the hypothesis finished: </s> is not part of the answer
                break
            piece = lib.amd_token_piece(ctx, int(t))
            text += piece
            if ignore_eos:
                shown += piece
            elif lib.minigpt4_contains_eos_token(piece):
                pass
            elif lib.minigpt4_is_eos(text):
                break
            else:
                shown += piece
        return shown

    def _run(self, requests, answers, temp, top_k, top_p, ignore_eos, batched_prefill, logprobs, penalised, logit_bias, pen, num_beams=1, length_penalty=1.0, guidance=None, negative_prompt=None, sessions=None, seeds=None, chain=None, lookup=0) -> List[str]:
        import ctypes
        lib, ctx = self.lib, self.ctx
        if lookup and not self._speculation:
            lib.amd_set_speculation(ctx, 7)
            self._speculation = True
        if penalised:
            lib.amd_set_penalties(ctx, True)
        self.last_logprobs = [[] for _ in requests] if logprobs > 0 else None
        per = 2 if guidance is not None else num_beams            # conversations per request: its own, then the guidance conversation / the search's scratch
        for wave in plan_waves(len(requests), self.conversations // per):
            structs, owned, emb_of = [], [], {}
            for i in wave:
                if requests[i].image is None:                 # a follow-up turn: its image rows are in the parked snapshot
                    continue
                st, own = self._to_struct(requests[i].image)
                emb_of[i] = len(structs)
                structs.append(st)
                owned += own
            arr = (ML.MiniGPT4Image * max(len(structs), 1))(*structs)
            batch, embs = ML.MiniGPT4Images(arr, len(structs)), ML.MiniGPT4Embeddings()
            if structs:
                lib.panic_if_error(lib.library.minigpt4_amd_encode_images(ctx.ptr, ctypes.byref(batch), ctypes.byref(embs), 0))
            try:
                for j, i in enumerate(wave):
                    slot = j * per
                    lib.amd_select_conversation(ctx, slot)
                    if requests[i].image is None:
                        self.resume(slot, self._parked[sessions[i]])   # the parked blob stays until the wave has parked the session again: a failure in between loses nothing
                        lib.minigpt4_begin_chat(ctx, requests[i].prompt)
                    else:
                        lib.minigpt4_reset_chat(ctx)
                        lib.minigpt4_system_prompt(ctx)
                        lib.minigpt4_begin_chat_image(ctx, embs.embeddings[emb_of[i]], requests[i].prompt)
                    if penalised:
                        lib.amd_conversation_penalties(ctx, slot, **pen)
                    if logit_bias:
                        lib.amd_set_logit_bias(ctx, logit_bias)
                    if self._constraint:
                        lib.amd_set_constraint(ctx, slot, self._constraint)   # (also returns the state to the start)
                    if seeds is not None:
                        lib.amd_conversation_seed(ctx, slot, seeds[i], 0)     # the request's own stream, from its first draw
                        if chain is not None:
                            lib.amd_conversation_mirostat(ctx, slot, None)    # and its own mu, unset
                    if guidance is not None:                  # the guidance conversation: the same question (or the negative prompt) asked without the image
                        lib.amd_select_conversation(ctx, slot + 1)
                        lib.minigpt4_reset_chat(ctx)
                        lib.minigpt4_system_prompt(ctx)
                        lib.minigpt4_begin_chat(ctx, requests[i].prompt if negative_prompt is None else negative_prompt)
                if batched_prefill:                           # the wave's prompts in one pass per chunk instead of one pass per conversation
                    lib.amd_prefill_batch(ctx, [j * per + k for j in range(len(wave)) for k in range(2 if guidance is not None else 1)])
                if num_beams > 1:
                    for j, i in enumerate(wave):
                        answers[i] = self._beam_answer(list(range(j * per, (j + 1) * per)), requests[i].max_tokens, length_penalty, ignore_eos)
                    continue
                text = {slot: "" for slot in range(len(wave))}
                shown = {slot: "" for slot in range(len(wave))}
                left = {slot: requests[i].max_tokens for slot, i in enumerate(wave)}
                active = [slot for slot in range(len(wave)) if left[slot] > 0]

                def take(slot, piece):                        # THE stop rule, one piece at a time, for both loops below: True = the request is done
                    left[slot] -= 1
                    text[slot] += piece
                    done = left[slot] <= 0
                    if self._constraint:                          # the pattern decides: the answer ends where the constraint let "</s>" through
                        if piece == "</s>":
                            done = True
                        else:
                            shown[slot] += piece
                    elif not ignore_eos:
                        if lib.minigpt4_contains_eos_token(piece):
                            pass                                  # swallowed, like the reference's `continue`
                        elif lib.minigpt4_is_eos(text[slot]):
                            done = True
                        else:
                            shown[slot] += piece
                    else:
                        shown[slot] += piece
                    return done
                if lookup:                                    # the drafter's history per request: its prompt's tokens, then what it emits; the token that comes next
                    corpus = {slot: lib.amd_tokenize(ctx, requests[i].prompt.encode("utf-8"), add_bos=False) for slot, i in enumerate(wave)}
                    coming = {slot: None for slot in range(len(wave))}
                while active and lookup:
                    spare, drafts = getattr(self, "_row_cap", 64) - len(active), []   # draft rows the pass holds beside one row per request: later drafts are shortened
                    for slot in active:
                        d = [] if coming[slot] is None else ngram_draft(corpus[slot] + [coming[slot]], n_draft=min(lookup, left[slot] - 1, spare))
                        spare -= len(d)
                        drafts.append(d)
                    step = lib.amd_verify_draft_batch(ctx, active, drafts)
                    nxt = []
                    for r, slot in enumerate(active):
                        ids = [int(t) for t in step["ids"][r]]
                        done = not ids                            # a full context that cannot shift: the request ends here
                        if ids:
                            coming[slot] = int(step["row_greedy"][r][len(ids) - 1])
                        for t in ids:                             # piece by piece; what was kept behind the stop is discarded
                            corpus[slot].append(t)
                            done = take(slot, lib.amd_token_piece(ctx, t))
                            if done:
                                break
                        if not done:
                            nxt.append(slot)
                    active = nxt
                while active:
                    if logprobs > 0:
                        step = lib.amd_end_chat_batch_top(ctx, active, top_n=logprobs, temp=temp, top_k=top_k, top_p=top_p)
                        pieces = step["pieces"]
                        for r, slot in enumerate(active):
                            self.last_logprobs[wave[slot]].append(dict(
                                id=int(step["ids"][r]), piece=pieces[r], logprob=float(step["logprob"][r]), rank=int(step["rank"][r]),
                                top=[(lib.amd_token_piece(ctx, int(t)), float(v)) for t, v in zip(step["top_ids"][r], step["top_logprobs"][r])]))
                    elif guidance is not None:
                        pieces = lib.amd_end_chat_guided(ctx, [2 * slot for slot in active], [2 * slot + 1 for slot in active], guidance, temp=temp, top_k=top_k, top_p=top_p)
                    elif seeds is not None:
                        pieces = lib.amd_end_chat_batch_sampled(ctx, active, temp=temp, top_k=top_k, top_p=top_p, **(chain or {}))
                    else:
                        pieces = lib.amd_end_chat_batch(ctx, active, temp=temp, top_k=top_k, top_p=top_p)
                    nxt = []
                    for slot, piece in zip(active, pieces):
                        if not take(slot, piece):
                            nxt.append(slot)
                    active = nxt
                for slot, i in enumerate(wave):
                    answers[i] = shown[slot]
                    if sessions is not None and sessions[i] is not None:
                        self._parked[sessions[i]] = self.suspend(slot)
            finally:
                if structs:
                    lib.library.minigpt4_amd_free_embeddings(ctypes.byref(embs))
                for im in owned:
                    lib.minigpt4_free_image(im)
        lib.amd_select_conversation(ctx, 0)
        return answers


def serve(requests: Sequence[Request], vision_path: str, llm_path: str, conversations: int = 4, **kw) -> Optional[List[str]]:
    """Data-parallel entry point: call it on every rank of a `torch.distributed` job (or alone).  Rank r serves requests r, r + world, ...;
    rank 0 returns all answers in request order, the other ranks return None.  With world > 1 the replicas are loaded through `dist.load_replica`
    (file load on rank 0, arena broadcast to the others); pass `device=torch.device("cuda", local_rank)` on GPUs."""
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    mine = D.shard_requests(len(requests), rank, world)
    if kw.get("seeds") is not None and len(kw["seeds"]) != len(requests):
        raise ValueError("seeds: one integer per request")
    server = ReplicaServer(vision_path, llm_path, conversations=conversations, rank=rank, world=world, device=kw.get("device"),
                           **{k: v for k, v in kw.items() if k in ("n_ctx", "n_batch", "seed", "library", "verbosity", "prefix_cache")})
    try:
        out = server.run([requests[i] for i in mine], **{k: v for k, v in kw.items() if k in ("temp", "top_k", "top_p", "ignore_eos", "logprobs", "repeat_penalty", "repeat_last_n",
                                                                                                "presence_penalty", "frequency_penalty", "logit_bias", "num_beams",
                                                                                                "length_penalty", "guidance_scale", "negative_prompt", "regex", "device_sampling",
                                                                                                "tfs_z", "typical_p", "min_p", "mirostat", "mirostat_tau", "mirostat_eta", "lookup")},
                         **({"seeds": [(kw["seeds"][i] if kw.get("seeds") is not None else i) for i in mine]} if kw.get("device_sampling") or kw.get("seeds") is not None else {}))   # a request's seed follows it to its rank
    finally:
        server.close()
    mapping = dict(zip(mine, out))
    if world == 1:
        return merge_answers(len(requests), [mapping])
    per_rank = D.gather_objects(mapping, world)            # a collective: every rank calls it exactly once
    return merge_answers(len(requests), per_rank) if rank == 0 else None


def merge_answers(n_requests: int, per_rank: Sequence[dict]) -> List[str]:
    merged = {}
    for d in per_rank:
        merged.update(d)
    assert sorted(merged) == list(range(n_requests)), "every request must be answered by exactly one rank"
    return [merged[i] for i in range(n_requests)]
