"""The two benchmarked step schedules of `Trainer.forward_backward`: forward AND backward as two chains without autograd
(`_AlignerEngine._run_chains`).  `_ChainStep` is what both share; `Stage1Step` ('init') and `Stage2Step` ('cotrain') hold what differs;
`HandOver` is how stage 2's two issuing host threads meet."""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

from . import _lib, dist, ops
from .loss import (SimFam, _Blocks, _diag_max, _ManualCtx, _NCETail, _p, _pos_masks, _side_stream, agreement_targets, nce_family_stages,
                   nce_term_grads, prepare_inputs_async, stage2_masks)


def text_pad_bool(batch):
    """the [B, N] sentence padding mask as bool (train/main.py:86 passes .bool() every step; `to_device_batch` converts it once)"""
    return batch["_text_pad_bool"] if batch.get("_text_pad_bool") is not None else batch["text_padding_mask"].bool()


class HandOver:
    """Host-side hand-overs between the two threads that issue a step's chains: a stream event can only be waited for once it has
    been recorded, so the recording thread publishes it under a name and the other one waits for that name.  Pure `threading`: the
    event is an opaque object.  A chain that fails says so, which wakes every waiter: it must not wait out its timeout."""

    def __init__(self, names, timeout=120.0):
        self.timeout, self._events, self._failed = timeout, {}, []
        self._flags = {k: threading.Event() for k in names}

    def publish(self, name, event):
        self._events[name] = event
        self._flags[name].set()

    def wait(self, name):
        if not self._flags[name].wait(timeout=self.timeout) or self._failed:
            err = _lib.TanHipError(f"stage-2 step: the other chain did not reach '{name}'"
                                   + (f" ({self._failed[0]} chain failed)" if self._failed else ""))
            err.tan_consequence = True          # (`_run_chains` reports the other thread's error instead)
            raise err
        return self._events[name]

    def fail(self, chain):
        self._failed.append(chain)
        for f_ in self._flags.values():
            f_.set()


def _guarded(method):          # a chain's method `(self, which, ...)`: its failure is handed over to the other chain's thread
    def run(self, which, *args, **kw):
        try:
            return method(self, which, *args, **kw)
        except BaseException:
            self.sync.fail(which)
            raise
    return run


class _ChainStep:
    """What both schedules share: everything the loss derives from the batch alone on the loss side stream, the masks, the gradient
    fill's event, the optimizer / data-parallel callbacks behind each stack's backward, the call into `_run_chains`, the language
    model's backward and the events a pipelined step hands back to `Trainer.step`.  A schedule adds `family` and `finish`, and `mid()`
    or `pre(which)` for `_run_chains` (methods, not attributes that hold them: the step must not keep itself alive in a cycle)."""
    mid = pre = None

    def __init__(self, tr, batch):
        self.tr, self.batch, self.a, self.m = tr, batch, tr.args, tr.online
        self.video, self.lang = video, lang = batch["video"], batch["text_embed"]
        self.B, self.T, self.N, self.dev = video.shape[0], video.shape[1], lang.shape[1], video.device
        self.Se, self.Sd = self.m.num_encoder_layers, self.m.num_decoder_layers
        self.main, self.ls = torch.cuda.current_stream(), _side_stream(self.dev)
        self.prep = prepare_inputs_async(batch, batch["padding_mask"], batch["text_padding_mask"], self.T, self.N, self.dev, self.a,
                                         batch.get("n_text"), want_compaction=True)
        self.nv = self.prep.get("nv")
        self.vmask, self.tmask = self.m._mask_u8(batch["padding_mask"]), self.m._mask_u8(text_pad_bool(batch))

    def run(self):
        tr, m, lang = self.tr, self.m, self.lang
        pipe = None
        if tr._in_step and m._flat.in_step:
            pipe = {"zero": tr._zero_ev}                 # (each chain waits for the fill in front of its first backward kernel)
        elif tr._zero_ev is not None:                    # the gradient buffer's fill ran on a side stream
            self.main.wait_event(tr._zero_ev)
        tr._zero_ev = None
        after_v = after_j = None
        if tr._in_step:
            early = os.environ.get("TAN_OPT_EARLY", "1") != "0" and tr._early_ok()
            ddp, gs = tr._ddp, 1.0 / dist.world_size()

            def stack_done(which):
                # (main host thread, current stream = the one that carries the stack's last weight gradients) data parallel: the stack's
                # slice of the gradient is summed over ranks first; then its matrices may be stepped
                reduced = ddp.stack_done(which) if ddp is not None else True
                if ddp is not None:
                    # the remainder's optimizer launch (main stream) reads this stack's bias / LayerNorm gradients: behind the stack's
                    # collective AND the bf16 wire's cast back to f32, which run on this role stream
                    ddp.stack_events[which] = torch.cuda.current_stream().record_event()
                if early and reduced:
                    tr.early_update(which, gs)
            if early or ddp is not None:
                after_v, after_j = (lambda: stack_done("video")), (lambda: stack_done("joint"))       # noqa: E731
        pre = None if self.pre is None else {"video": lambda: self.pre("video"), "joint": lambda: self.pre("joint")}
        res = m._run_chains(self.video, lang, self.vmask, self.tmask, self.family, after_v, after_j, pipe=pipe, mid=self.mid,
                            need_d_lang=lang.requires_grad, pre=pre)
        if lang.requires_grad:
            # the step started from token ids: the sentence embeddings' gradient (the embeddings' backward produced it) goes on through
            # the language model under autograd (index_select of `embed_sentences`, Word2VecModel's HIP nodes), on this stream
            lang.backward(res.d_lang.to(lang.dtype))
        tr._pipe_out = res.out_ev                        # (None unless pipelined)
        return self.finish(res)


class Stage1Step(_ChainStep):
    """Stage 1 ('init'): the loss is (loss_dual + loss_joint) / 2 with weights that depend on the batch's masks only, so the terms'
    upstream gradients are known up front and the chains never wait for each other."""

    def __init__(self, tr, batch, terms_timeout=60.0):
        super().__init__(tr, batch)
        self.terms_timeout, self.out, prep = terms_timeout, None, self.prep
        with torch.cuda.stream(self.ls):                 # the gradients of the NCE terms, on the loss side stream too
            self.cols_tail = prep["cols_pos_c"] if self.nv is not None else prep["cols_pos"]
            self.g = nce_term_grads(prep["rows_pos"], self.cols_tail, self.Se, self.Sd)[:4]        # g_v_d, g_t_d, g_v_j, g_t_j
            self.ready = self.ls.record_event()
        self.tgt, self.ci = prep["tgt"], prep["tpad_u8"].view(self.B * self.N)

    def family(self, which, x_video, v_grp, x_text, t_grp, d_video, d_text):
        torch.cuda.current_stream().wait_event(self.ready)          # (a finished event costs nothing)
        gv, gt = self.g[:2] if which == "dual" else self.g[2:]
        return nce_family_stages(x_video, v_grp, x_text, t_grp, d_video, d_text, self.tgt, self.ci, self.B, self.T, self.N, self.nv, gv, gt)

    def mid(self, v_d, t_d, terms, ready):
        # the masked means of the four term tensors (loss.py:254-275), on the main stream right behind the video stack's backward:
        # the joint family's terms were final ~1.5 ms earlier on their stream; issued at the end of the step the launch sat between
        # the embeddings' backward and the optimizer launch (4.126 -> 4.078 ms per step, ABBA x2 of 60 steps)
        if not ready.wait(timeout=self.terms_timeout) or not terms:
            raise _lib.TanHipError("the joint chain did not reach its loss family")      # (`_run_chains` re-raises the chain's own error)
        v_j, t_j, ev_j = terms[0]
        self.main.wait_event(ev_j)
        for t in (v_j, t_j):
            t.record_stream(self.main)
        self.out = _NCETail.forward(_ManualCtx(), v_d, t_d, v_j, t_j, self.prep["rows_pos"], self.cols_tail, None)

    def finish(self, res):
        for t in (*self.g, self.cols_tail, self.prep["rows_pos"], res.v_j, res.t_j):
            t.record_stream(self.main)
        return dict(zip(("loss-dual", "loss-joint", "loss"), self.out))


class Stage2Step(_ChainStep):
    """Stage-2 co-training step (train/main.py:89-98,122; train/loss.py:88-229,277-373) as two chains without autograd:
        main:  EMA video stack -> cosines | online video stack -> sweep(dual)  .. finish(dual)  .. backward(dual)  -> stack backward
        side:  EMA joint stack -> cosines | online joint stack -> head -> sweep(joint) .. finish(joint) .. backward(joint) + head -> stack backward
    with two meeting points: (1) the agreement targets need both EMA stacks' same-video cosines (small launches on the loss stream,
    issued by the main chain's host thread: they are through long before the online sweeps are); (2) the terms' upstream gradients
    need both families' forward results -- per-sentence maxima -> z-scores / quantile threshold / kept rows, alignability labels,
    BCE (train/loss.py:277-357) -- issued on the main chain's stream between its family's finishing launch and backward.
    Every launch is the one `get_loss` issues on the autograd path (same kernels, `tan_simfam_*` for the families)."""
    Cw = 512

    def __init__(self, tr, batch, timeout=120.0):
        super().__init__(tr, batch)
        B, T, N, dev, Se, Sd = self.B, self.T, self.N, self.dev, self.Se, self.Sd
        self.tg = tg = tr.model.target
        R, Mp = B * T, B * N
        self.R, self.Mp, self.L = R, Mp, T + N
        self.Mc = Mc = self.nv[0].shape[0] if self.nv is not None else Mp
        self.tpad_u8, self.ci = self.prep["tpad_u8"], self.prep["tpad_u8"].view(Mp)
        # buffers that the meeting points fill (their addresses go into the families' descriptors up front)
        self.tgt = torch.empty(B, T, N, device=dev)
        self.g = {"dual": (torch.empty(Se, R, device=dev), torch.empty(Se, Mc, device=dev)),
                  "joint": (torch.empty(Sd, R, device=dev), torch.empty(Sd, Mc, device=dev))}
        self.d_head = torch.empty(Mp, device=dev)               # d loss / d alignability logits of joint stage 2 (train/loss.py:341)
        self.sync = HandOver(("ema_video", "ema_joint", "tgt", "fin_joint", "g"), timeout)
        self.fams, self.ema_diag, self.aux = {}, {}, {}          # per family: its SimFam, the EMA stack's cosines; what `last_aux` keeps
        self.jt = self.a_j2 = self.md = self.mj = None           # the head's input rows and logits; per-sentence maxima of dual / joint
        # ---- the EMA target (tan_model.py:346-351 `forward_from_ema`, no gradient): its input embeddings here, its stacks on the chains
        with torch.no_grad():
            tg._ensure_flat()
            self.fe_t = tg._embed_fused(self.video, self.lang, self.vmask, self.tmask, 0, 0, 0, False)

    @_guarded
    def pre(self, which):
        cur = torch.cuda.current_stream()
        with torch.no_grad():
            self.ema_diag[which] = self.tg._ema_stack_diag(which, self.fe_t, self.vmask, self.tmask, self.B, self.T, self.N)
        self.sync.publish("ema_" + which, cur.record_event())

    def targets(self):
        # meeting point 1, on the loss stream: train/loss.py:88-229 (self-labelling of both EMA families, agreement 'keep' / ...,
        # de-duplication) + the positive masks of loss.py:236-237
        ls, prep, nv, tgt, B, T, N = self.ls, self.prep, self.nv, self.tgt, self.B, self.T, self.N
        ev_ema_joint = self.sync.wait("ema_joint")       # (the other thread's; "ema_video" is this one's own)
        for ev in (self.sync.wait("ema_video"), ev_ema_joint, prep["_event"]):
            ls.wait_event(ev)
        with torch.cuda.stream(ls):
            for t_ in self.ema_diag.values():
                t_.record_stream(ls)
            J, D, _, iou, conf = agreement_targets(_Blocks.of_diag(self.ema_diag["joint"]), _Blocks.of_diag(self.ema_diag["video"]), prep,
                                                   B, T, N, self.a.temporal_agreement_type, tgt=tgt)
            rows_pos, cols_pos = _pos_masks(tgt, self.tpad_u8, B, T, N)
            cols_tail = cols_pos.index_select(0, nv[0]) if nv is not None else cols_pos
            ev_tgt = ls.record_event()
        self.aux.update(max_position_joint=J["max_pos"], max_position_dual=D["max_pos"], max_logits_joint=J["max_logit"],
                        max_logits_dual=D["max_logit"], joint_self_tgt=J["tgt"], dual_self_tgt=D["tgt"], iou=iou, confidence_mask=conf,
                        agreement_tgt=tgt, rows_pos=rows_pos, cols_tail=cols_tail)
        self.sync.publish("tgt", ev_tgt)

    def upstream(self):
        # meeting point 2, on the main chain's stream: train/loss.py:277-357 and the tail's backward
        lib, dev, g, nv, Se, Sd, R, Mc, Mp = _lib.lib(), self.dev, self.g, self.nv, self.Se, self.Sd, self.R, self.Mc, self.Mp
        cur = torch.cuda.current_stream()
        fd, fj = self.fams["dual"], self.fams["joint"]
        fj.record_stream(cur)
        md, mj = self.md, self.mj                # per-sentence maxima (loss.py:280,283): each chain's own launch behind its finish
        mj.record_stream(cur)
        s2 = stage2_masks(md, mj, self.tpad_u8, self.tgt, self.batch.get("abs_text_pos"), self.aux["confidence_mask"], self.a.loss_threshold,
                          True, self.B, self.T, self.N)
        cols_th = s2["th_f"].index_select(0, nv[0]) if nv is not None else s2["th_f"]
        out_th = torch.empty(5, device=dev)              # [loss_dual_th, loss_joint_th, their mean, n_rows, n_cols]
        _lib.check(lib.tan_nce_tail_fwd(_p(fd.v_terms), _p(fd.t_terms), _p(fj.v_terms), _p(fj.t_terms), _p(s2["rows"]), _p(cols_th),
                                        C.c_int(Se), C.c_int(Sd), C.c_long(R), C.c_long(Mc), _p(out_th), _p(out_th[3:]), None,
                                        ops._stream()), "tan_nce_tail_fwd")
        one, gb = self.tr._stage2_consts(dev)
        _lib.check(lib.tan_nce_tail_bwd(None, None, _p(one), _p(s2["rows"]), _p(cols_th), _p(out_th[3:]), C.c_int(Se), C.c_int(Sd),
                                        C.c_long(R), C.c_long(Mc), _p(g["dual"][0]), _p(g["dual"][1]), _p(g["joint"][0]),
                                        _p(g["joint"][1]), ops._stream()), "tan_nce_tail_bwd")
        # BCE of the alignability head on joint stage 2 (loss.py:341-349), forward and backward
        a_joint = self.a_j2
        a_joint.record_stream(cur)
        bce = torch.empty(2, device=dev)
        _lib.check(lib.tan_bce_sel_fwd(_p(a_joint), _p(s2["y"]), _p(s2["sel"]), _p(s2["scal"]), C.c_int(Mp), _p(bce), ops._stream()),
                   "tan_bce_sel_fwd")
        _lib.check(lib.tan_bce_sel_bwd(_p(a_joint), _p(s2["y"]), _p(s2["sel"]), _p(s2["scal"]), _p(gb), C.c_int(Mp), _p(self.d_head),
                                       ops._stream()), "tan_bce_sel_bwd")
        self.sync.publish("g", cur.record_event())
        self.aux.update(t_th_mask=s2["th_mask"], max_logits_dual_per_text=md, max_logits_joint_per_text=mj, t_align_th_mask=s2["lab"],
                        out_th=out_th, bce=bce, s2=s2)

    @_guarded
    def family(self, which, x_video, v_grp, x_text, t_grp, d_video, d_text):
        m, sync, dev, B, T, N, Mp, L, Cw = self.m, self.sync, self.dev, self.B, self.T, self.N, self.Mp, self.L, self.Cw
        cur = torch.cuda.current_stream()
        cur.wait_event(self.prep["_event"])
        fam = self.fams[which] = SimFam(x_video, v_grp, x_text, t_grp, d_video, d_text, self.tgt, self.ci, B, T, N, self.nv, *self.g[which])
        fam.sweep()
        if which == "joint":
            # alignability head on the text rows of joint stage 2 (tan_model.py:147-148; the only stage the loss reads, loss.py:341)
            self.jt = torch.empty(Mp, Cw, dtype=x_text[2].dtype, device=dev)
            ops.rows_copy(x_text[2], self.jt, B, N, Cw, L, T, N, 0)
            self.a_j2 = torch.empty(Mp, device=dev)
            ops.head_fwd(self.jt, m._f("binary_head.weight").view(-1), m._f("binary_head.bias"), self.a_j2, Mp, Cw)
            cur.wait_event(sync.wait("tgt"))
            fam.finish()
            self.mj = _diag_max(_Blocks.of_diag(fam.diag_last), None, B, T, N)
            sync.publish("fin_joint", cur.record_event())
            cur.wait_event(sync.wait("g"))
        else:
            self.targets()
            cur.wait_event(sync.wait("tgt"))
            fam.finish()
            self.md = _diag_max(_Blocks.of_diag(fam.diag_last), None, B, T, N)
            cur.wait_event(sync.wait("fin_joint"))
            self.upstream()
        fam.backward()
        if which == "joint":
            d_jt = torch.empty(Mp, Cw, dtype=self.jt.dtype, device=dev)
            ops.head_bwd(self.d_head, self.jt, m._f("binary_head.weight").view(-1), d_jt, m._g("binary_head.weight").view(-1),
                         m._g("binary_head.bias"), Mp, Cw)
            ops.rows_copy(d_jt, d_text[2], B, N, Cw, N, 0, L, T, accumulate=True)
            self.d_head.record_stream(cur)
        return fam.v_terms, fam.t_terms

    def finish(self, res):
        lib, dev, main, ls, aux, tr = _lib.lib(), self.dev, self.main, self.ls, self.aux, self.tr
        self.tg._release_ws(self.fe_t["em"])
        # ---- the loss dictionary (monitoring entries on the loss stream; train/loss.py:296-304,359-373)
        fd, fj = self.fams["dual"], self.fams["joint"]
        out_th, bce, s2 = aux.pop("out_th"), aux.pop("bce"), aux.pop("s2")
        with torch.cuda.stream(ls):
            ls.wait_event(self.sync.wait("g"))
            for f_ in (fd, fj):
                f_.record_stream(ls)
            out_all = torch.empty(5, device=dev)
            _lib.check(lib.tan_nce_tail_fwd(_p(fd.v_terms), _p(fd.t_terms), _p(fj.v_terms), _p(fj.t_terms), _p(aux["rows_pos"]),
                                            _p(aux["cols_tail"]), C.c_int(self.Se), C.c_int(self.Sd), C.c_long(self.R), C.c_long(self.Mc),
                                            _p(out_all), _p(out_all[3:]), None, ops._stream()), "tan_nce_tail_fwd")
            loss = out_th[2] + bce[0]
        main.wait_stream(ls)
        # (allocator bookkeeping for what crossed streams: main joined `ls` just above and joined the side stream inside `_run_chains`,
        #  so a block freed after this point is safe for main's allocator; what was allocated under `ls` / the side stream and read on
        #  main is recorded here -- a minimal set: ~130 record_stream calls cost 0.13 ms of host time at the end of every step)
        for t_ in (out_all, loss, aux["confidence_mask"], self.mj, self.a_j2):
            t_.record_stream(main)
        for t_ in self.prep["_tensors"]:
            t_.record_stream(main)
        fj.record_stream(main)
        if tr.keep_aux:
            tr.last_aux = {k: v for k, v in aux.items() if k not in ("rows_pos", "cols_tail")}
        return {"loss-dual": out_th[0], "loss-joint": out_th[1], "loss-dual-all": out_all[0], "loss-joint-all": out_all[1],
                "loss-total": out_all[2], "loss-joint-bce": bce[0], "alignability_top1": bce[1], "confidence-ratio": s2["scal"][3],
                "iou-threshold": torch.full((), 0.5, device=dev), "loss": loss}
