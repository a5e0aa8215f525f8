"""What the wrappers of cgs_amd/kernels.py hand to the C ABI: one fixed, seeded script that calls every public wrapper through its
public API, and a recorder of every library call the script causes.  Not a test module and not a conftest: test_gpu_abi_trace.py runs
this file in a fresh process and holds the result to tests/golden/abi_trace.json.

The script.  Every conv-family wrapper once per form (plain / stats / nstats / signs / update) at B = 2 on 8 x 8 grids, the smallest
shapes at which the library offers each form (asked of conv_signs_ok / conv_stat_layout / conv_update_form first); linear_* at N = 1
and N > 1; pool_moments with rows= and shift=; mh_walk / compact_rows with take_all, fill and capacity.  It runs three times on the
same tensors: plain, with ``K.PROFILE = {}``, and with ``K.PROFILE_BY_LAYER`` too (of that pass only the records are kept).

A record is ``[entry name, [arguments], return value]``.  A device pointer becomes the label of the script tensor with that
``data_ptr()`` -- tensors a wrapper returns are labelled ``<step>.<i>`` -- any other pointer that stands where a scratch area does
(before its byte count) ``ws<k>``, numbered by first appearance, and what is left (a wrapper's own temporary) ``"tmp"``; the stream ``"s"``; a ``LadamSeed`` byref its fields; the ints the two layout queries write through pointers their values;
ints and floats stay as they are.  ``cgs_adam_multi`` also carries the slot table and the chunk plan read back from the device.

The trace is that of a FRESH process (which workspace queries are asked, what is packed, how large the grow-only scratch is, all
depend on what ran before), hence the command line:  python tests/abi_trace_cases.py OUT.json"""
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_trace.json")
HOST_OUT = {"cgs_conv_stat_layout": 3, "cgs_conv_update_form": 1}       # trailing pointer arguments that are host ints the query writes
WS_FIRST = ("cgs_bn_train_param_grads", "cgs_instnorm_param_grads")     # entry points that read a scratch area as their first argument


def kernels_source_names():
    """Every entry point kernels.py names: as a string handed to ``lib.call`` or as an attribute of the loaded library."""
    with open(os.path.join(ROOT, "collaborative-gan-sampling_amd", "kernels.py")) as f:
        src = f.read()
    return set(re.findall(r'"(cgs_\w+)"', src)) | set(re.findall(r'\.(cgs_\w+)\(', src))


def prepacked_index(name, signatures):
    """Position of ``ws_prepacked`` in the entry point's arguments (the int that follows the workspace's size_t), or None."""
    args = signatures[name][1]
    hits = [i + 1 for i in range(len(args) - 1) if args[i] is C.c_size_t and args[i + 1] is C.c_int]
    return hits[0] if hits else None


def is_launch(name, signatures):
    """An entry point that takes a stream (its last argument)."""
    args = signatures[name][1]
    return bool(args) and args[-1] is C.c_void_p and name not in HOST_OUT


class _Ptr:
    def __init__(self, value, scratch=False):
        self.value, self.scratch = value, scratch


class Recorder:
    """Stands in for the loaded library (``lib._lib``): every ``cgs_*`` call goes through to it and leaves a record."""

    def __init__(self, real, signatures):
        self._real, self._sig = real, signatures
        self.records = []          # of the pass being recorded
        self._open = []            # records of the running step: their pointers are labelled when it ends
        self.labels = {}           # data_ptr -> label of a script tensor
        self.tensors = {}          # label -> tensor
        self._keep = []            # every tensor ever labelled stays alive: no address is handed out twice
        self.ws = {}               # any other pointer -> ws<k>

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("cgs_"):
            return fn

        def traced(*args):
            ret = fn(*args)
            self._note(name, args, ret)
            return ret
        return traced

    def _note(self, name, args, ret):
        types = self._sig[name][1]
        out = []
        for i, (a, ty) in enumerate(zip(args, types)):
            if ty is not C.c_void_p:
                out.append(a)
            elif a is None:
                out.append(None)
            elif name in HOST_OUT and i >= len(types) - HOST_OUT[name]:
                out.append(C.c_int.from_address(a).value)
            elif i == len(types) - 1:
                out.append("s")
            elif hasattr(a, "_obj"):                                      # byref(LadamSeed)
                s = a._obj
                out.append({"LadamSeed": [_Ptr(s.s_real), _Ptr(s.loss_avg), _Ptr(s.gain), s.first]})
            else:
                out.append(_Ptr(int(a), types[i + 1] is C.c_size_t or (i == 0 and name in WS_FIRST)))
        rec = [name, out, ret.decode() if isinstance(ret, bytes) else ret]
        if name == "cgs_adam_multi":
            rec.append(self._adam_tables(args))
        self.records.append(rec)
        self._open.append(rec)

    def _adam_tables(self, args):
        import numpy as np
        table = self.tensors[self.labels[args[0]]].cpu().numpy().view(np.dtype([("w", "<u8"), ("g", "<u8"), ("m", "<u8"), ("v", "<u8"), ("n", "<u8")]))
        plan = self.tensors[self.labels[args[2]]].cpu().numpy().view(np.dtype([("slot", "<i4"), ("count", "<u4"), ("begin", "<u8")]))
        return {"table": [[_Ptr(int(r[k])) for k in ("w", "g", "m", "v")] + [int(r["n"])] for r in table],
                "plan": [[int(r["slot"]), int(r["count"]), int(r["begin"])] for r in plan]}

    def add(self, label, t):
        self.tensors[label] = t
        self._keep.append(t)
        self.labels[t.data_ptr()] = label
        return t

    def _label(self, v):
        if isinstance(v, _Ptr):
            hit = self.labels.get(v.value)
            if hit is not None:
                return hit
            return self.ws.setdefault(v.value, f"ws{len(self.ws)}") if v.scratch else "tmp"
        if isinstance(v, dict):
            return {k: self._label(x) for k, x in v.items()}
        if isinstance(v, (list, tuple)):
            return [self._label(x) for x in v]
        return v

    def close_step(self):
        for rec in self._open:
            rec[1:] = self._label(rec[1:])
        self._open = []


def _tensors(R, dev):
    """The script's inputs, seeded; every one is registered under its name."""
    import torch
    g = torch.Generator().manual_seed(20190)

    def f32(name, *shape, scale=1.0, lo=None):
        t = torch.randn(shape, generator=g) * scale
        if lo is not None:
            t = t.abs() + lo
        return R.add(name, t.float().contiguous().to(dev))

    def f64(name, *shape):
        return R.add(name, torch.rand(shape, generator=g, dtype=torch.float64).to(dev))

    def empty(name, dtype, *shape, fill=0):
        return R.add(name, torch.full(shape, fill, dtype=dtype, device=dev))

    T = {}
    # conv 3x3 stride 1, 32 -> 64 channels on 8 x 8 (forward forms); its backward-data twin 64 <- 96
    T["cx"], T["cw"], T["cb"] = f32("cx", 2, 8, 8, 32), f32("cw", 3, 3, 32, 64, scale=0.05), f32("cb", 64, scale=0.1)
    T["cy"], T["ca"], T["cc"] = f32("cy", 2, 8, 8, 64), f32("ca", 64, lo=0.5), f32("cc", 64, scale=0.1)
    T["bdy"], T["bw"], T["bdx"] = f32("bdy", 2, 8, 8, 96), f32("bw", 3, 3, 64, 96, scale=0.05), f32("bdx", 2, 8, 8, 64)
    T["baux"], T["ba"] = f32("baux", 2, 8, 8, 64), f32("ba", 64, lo=0.5)
    T["nx"], T["ngamma"], T["nbeta"] = f32("nx", 2, 8, 8, 64), f32("ngamma", 64, lo=0.5), f32("nbeta", 64, scale=0.1)
    T["theta"], T["m"] = f32("theta", 2, 8, 8, 64), f32("m", 2, 8, 8, 64)
    # deconv 3x3 stride 2, 64 -> 32 channels, 8 x 8 -> 16 x 16 (plain, stats); 5x5 32 -> 32 (sign mask out)
    T["dx"], T["dw"], T["db"], T["dy"] = f32("dx", 2, 8, 8, 64), f32("dw", 3, 3, 32, 64, scale=0.05), f32("db", 32, scale=0.1), f32("dy", 2, 16, 16, 32)
    T["sx"], T["sw"], T["sb"], T["sy"] = f32("sx", 2, 8, 8, 32), f32("sw", 5, 5, 32, 32, scale=0.05), f32("sb", 32, scale=0.1), f32("sy", 2, 16, 16, 32)
    T["ssigns"] = empty("ssigns", torch.int32, 2 * 16 * 16 * 32 // 32)
    # deconv backward-data 5x5 stride 2: 128 <- 64 channels (plain, nstats, update); to 3 channels (sign mask in)
    T["ebdy"], T["ebw"], T["ebdx"] = f32("ebdy", 2, 16, 16, 64), f32("ebw", 5, 5, 64, 128, scale=0.05), f32("ebdx", 2, 8, 8, 128)
    T["enx"], T["engamma"], T["enbeta"] = f32("enx", 2, 8, 8, 128), f32("engamma", 128, lo=0.5), f32("enbeta", 128, scale=0.1)
    T["etheta"], T["em"] = f32("etheta", 2, 8, 8, 128), f32("em", 2, 8, 8, 128)
    T["pdy"], T["pw"], T["pdx"] = f32("pdy", 2, 16, 32, 3), f32("pw", 5, 5, 3, 32, scale=0.05), f32("pdx", 2, 8, 16, 32)
    T["paux"], T["pa"] = f32("paux", 2, 8, 16, 32), f32("pa", 32, lo=0.5)
    T["psigns"] = empty("psigns", torch.int32, 2 * 8 * 16 * 32 // 32, fill=0x55555555)
    # linear 40 -> 12 and 40 -> 1
    T["lx"], T["lw"], T["lb"], T["ly"] = f32("lx", 5, 40), f32("lw", 40, 12, scale=0.1), f32("lb", 12, scale=0.1), f32("ly", 5, 12)
    T["lw1"], T["lb1"], T["ly1"], T["ldx"] = f32("lw1", 40, 1, scale=0.1), f32("lb1", 1, scale=0.1), f32("ly1", 5, 1), f32("ldx", 5, 40)
    T["ldl"], T["llm"] = f32("ldl", 5, 1), f32("llm", 5)
    # refinement scalars: B = 5 samples of 12 features, 6 logits per sample
    T["logits"], T["dlogits"], T["lmean"] = f32("logits", 5, 6), f32("dlogits", 5, 6), f32("lmean", 5)
    T["rtheta"], T["rm"], T["rv"], T["rg"] = f32("rtheta", 5, 12), f32("rm", 5, 12), f32("rv", 5, 12, lo=0.1), f32("rg", 5, 12)
    T["rbest"], T["rrows"], T["rbrows"] = f32("rbest", 5, 12), f32("rrows", 5, 7), f32("rbrows", 5, 7)
    T["rlogit"], T["rblogit"] = f32("rlogit", 5), f32("rblogit", 5)
    T["rforced"], T["rbstep"] = empty("rforced", torch.int32, 5), f32("rbstep", 5)
    T["tickets"] = empty("tickets", torch.int32, 5)
    T["loss"], T["loss_avg"], T["gain"] = f32("loss", 5, lo=0.1), f32("loss_avg", 5, lo=0.1), f32("gain", 5, lo=0.1)
    T["loss1"] = f32("loss1", 1)
    # weight gradients
    T["gw"], T["gdw"], T["gbias"] = f32("gw", 3, 3, 32, 64), f32("gdw", 3, 3, 32, 64), f32("gbias", 64)
    T["g1x"], T["g1dy"], T["g1dw"] = f32("g1x", 2, 8, 8, 64), f32("g1dy", 2, 8, 8, 1), f32("g1dw", 4, 4, 64, 1)
    T["gdeconv"], T["glin"] = f32("gdeconv", 3, 3, 32, 64), f32("glin", 40, 12)
    T["dgamma"], T["dbeta"] = f32("dgamma", 64), f32("dbeta", 64)
    T["edgamma"], T["edbeta"] = f32("edgamma", 128), f32("edbeta", 128)
    T["aw"], T["ag"], T["am"], T["av"] = f32("aw", 3000), f32("ag", 3000), f32("am", 3000), f32("av", 3000, lo=0.1)
    T["aw2"], T["ag2"], T["am2"], T["av2"] = f32("aw2", 7), f32("ag2", 7), f32("am2", 7), f32("av2", 7, lo=0.1)
    T["mmean"], T["mvar"] = f32("mmean", 64), f32("mvar", 64, lo=0.5)
    # float64 state
    T["px"], T["pshift"] = f32("px", 64, 8), f32("pshift", 8, scale=0.1)
    T["psum"], T["pgram"] = empty("psum", torch.float64, 8), empty("pgram", torch.float64, 8, 8)
    T["qsum"], T["qgram"] = empty("qsum", torch.float64, 8), empty("qgram", torch.float64, 8, 8)
    T["fa"], T["fb"], T["fo"], T["fd"] = f64("fa", 8, 8), f64("fb", 8, 8), empty("fo", torch.float64, 8, 8), empty("fd", torch.float64, 8)
    T["score"] = R.add("score", torch.rand((48, 1), generator=g).float().to(dev))
    T["edges"] = R.add("edges", torch.linspace(0.0, 1.0 + 1e-8, 11, dtype=torch.float64).to(dev))
    T["cal"] = empty("cal", torch.float64, 3 * 11 + 11)
    T["x2"], T["cent"], T["modes"] = f32("x2", 48, 2), f64("cent", 4, 2), empty("modes", torch.float64, 4 + 3)
    T["axx"], T["axy"] = f32("axx", 6), f32("axy", 5)
    T["whiten"], T["kde"] = R.add("whiten", torch.tensor([2.0, 0.1, 1.5], dtype=torch.float64).to(dev)), empty("kde", torch.float64, 6 * 5 + 1)
    T["sums"] = empty("sums", torch.float64, 2, 64)
    T["unif"], T["drs"], T["mh"] = f64("unif", 48), empty("drs", torch.float64, 1), empty("mh", torch.float64, 2)
    T["rowsrc"], T["pool"] = f32("rowsrc", 48, 3), f32("pool", 20, 3)
    T["mask"] = R.add("mask", (torch.rand(48, generator=g) < 0.5).to(torch.uint8).to(dev))
    T["takeall"] = R.add("takeall", torch.tensor([0, 1, 0], dtype=torch.uint8).to(dev))
    T["total"], T["fill"] = empty("total", torch.int32, 1), empty("fill", torch.int64, 1)
    return T


def _script(K, L, R, T):
    """Every public wrapper of kernels.py.  ``step(name, fn)`` runs one wrapper call and labels what it returned ``name.<i>``."""
    import numpy as np
    import torch

    def step(name, fn):
        out = fn()
        outs = out if isinstance(out, (tuple, list)) else (out,)
        for i, t in enumerate(outs):
            if isinstance(t, torch.Tensor) and t.data_ptr() not in R.labels:
                R.add(f"{name}.{i}", t)
        R.close_step()
        return out

    def refused(fn):
        try:
            fn()
        except L.CgsError:
            R.close_step()
            return
        raise AssertionError("the call was expected to be refused")

    def part(name, rows, C_):
        return T.get(name) if name in T else T.setdefault(name, R.add(name, torch.zeros((rows, 2, C_), dtype=torch.float32, device=T["cx"].device)))

    NONE = L.EPI_NONE
    # ---- contraction mode, the plan's error path
    step("contraction", lambda: K.set_contraction(K.set_contraction("bx6")))
    with K.contraction("f32"):
        pass
    R.close_step()
    refused(lambda: K.conv_stat_partials((2, 8, 8, 32), (3, 3, 32, 64), 0, 0))
    # ---- conv forward: plain with an epilogue, the two statistics forms
    step("conv2d_fwd", lambda: K.conv2d_fwd(T["cx"], T["cw"], T["cb"], 1, 1, L.EPI_AFFINE_RELU, T["ca"], T["cc"], out=T["cy"]))
    step("conv2d_fwd.alloc", lambda: K.conv2d_fwd(T["cx"], T["cw"], T["cb"], 2, 2))
    G = K.conv_stat_partials((2, 8, 8, 32), (3, 3, 32, 64), 1, 1)
    lay = K.conv_stat_layout(L.CONV_FWD, 2, 8, 8, 32, 0, 0, 64, 3, 3, 1, 1, 1)
    R.close_step()
    assert G > 0 and lay is not None
    step("conv2d_fwd_stats", lambda: K.conv2d_fwd_stats(T["cx"], T["cw"], T["cb"], part("cpart", max(G, lay[0]), 64), 1, 1, out=T["cy"]))
    step("groupnorm_fwd_partials", lambda: K.groupnorm_lrelu_fwd_from_partials(T["cy"], T["cpart"], lay, 2, T["ngamma"], T["nbeta"], 0.2))
    step("bn_fwd_partials", lambda: K.bn_train_lrelu_fwd_from_partials(T["cy"], T["cpart"][:G], T["ngamma"], T["nbeta"]))
    # ---- conv backward-data: plain with an epilogue, nstats, update
    step("conv2d_bwd_data", lambda: K.conv2d_bwd_data(T["bdy"], T["bw"], (8, 8), 1, 1, out=T["bdx"], epilogue=L.EPI_RELU_BWD_AFFINE, ep_a=T["ba"], ep_aux=T["baux"]))
    step("conv2d_bwd_data.alloc", lambda: K.conv2d_bwd_data(T["bdy"], T["bw"], (8, 8), 1, 1))
    _, mean, invstd = step("instnorm_fwd", lambda: K.instnorm_lrelu_fwd(T["nx"], T["ngamma"], T["nbeta"], 0.2))
    blay = K.conv_stat_layout(L.CONV_BWD_DATA, 2, 8, 8, 64, 0, 0, 96, 3, 3, 1, 1, 1)
    R.close_step()
    assert blay is not None
    ns = K.NormBwdStats(T["nx"], mean, invstd, T["ngamma"], T["nbeta"], 0.2, 1, part("bpart", blay[0], 64), blay)
    step("conv2d_bwd_data.nstats", lambda: K.conv2d_bwd_data(T["bdy"], T["bw"], (8, 8), 1, 1, out=T["bdx"], nstat=ns))
    step("norm_bwd_partials.groups", lambda: K.norm_lrelu_bwd_from_partials(T["bdx"], T["nx"], ns, 2, out=T["bdx"]))
    assert K.conv_update_form(L.CONV_BWD_DATA, 2, 8, 8, 64, 0, 0, 96, 3, 3, 1, 1) is not None
    R.close_step()
    step("conv2d_bwd_data.update", lambda: K.conv2d_bwd_data(T["bdy"], T["bw"], (8, 8), 1, 1, update=K.FusedUpdate(T["theta"], T["m"], 0.1, 0.9, False)))
    # ---- deconv forward: plain with an epilogue, stats, signs
    step("deconv2d_fwd", lambda: K.deconv2d_fwd(T["dx"], T["dw"], T["db"], (16, 16), 2, 2, L.EPI_AFFINE_RELU, T["sb"], T["db"], out=T["dy"]))
    dlay = K.conv_stat_layout(L.DECONV_FWD, 2, 8, 8, 64, 16, 16, 32, 3, 3, 2, 2, 1)
    R.close_step()
    assert dlay is not None
    step("deconv2d_fwd.stats", lambda: K.deconv2d_fwd(T["dx"], T["dw"], T["db"], (16, 16), 2, 2, out=T["dy"], part=part("dpart", dlay[0], 32)))
    assert K.conv_signs_ok(L.DECONV_FWD, 2, 8, 8, 32, 16, 16, 32, 5, 5, 2, 2, L.EPI_LRELU)
    R.close_step()
    step("deconv2d_fwd.signs", lambda: K.deconv2d_fwd(T["sx"], T["sw"], T["sb"], (16, 16), 2, 2, L.EPI_LRELU, out=T["sy"], signs=T["ssigns"]))
    # ---- deconv backward-data: plain with an epilogue, signs, nstats, update
    step("deconv2d_bwd_data", lambda: K.deconv2d_bwd_data(T["pdy"], T["pw"], (8, 16), 2, 2, out=T["pdx"], epilogue=L.EPI_RELU_BWD_AFFINE, ep_a=T["pa"], ep_aux=T["paux"]))
    assert K.conv_signs_ok(L.DECONV_BWD_DATA, 2, 8, 16, 32, 16, 32, 3, 5, 5, 2, 2, L.EPI_LRELU_BWD)
    R.close_step()
    step("deconv2d_bwd_data.signs", lambda: K.deconv2d_bwd_data(T["pdy"], T["pw"], (8, 16), 2, 2, out=T["pdx"], epilogue=L.EPI_LRELU_BWD, ep_signs=T["psigns"]))
    _, emean, einvstd = step("bn_fwd", lambda: K.bn_train_lrelu_fwd(T["enx"], T["engamma"], T["enbeta"]))
    elay = K.conv_stat_layout(L.DECONV_BWD_DATA, 2, 8, 8, 128, 16, 16, 64, 5, 5, 2, 2, 2)
    R.close_step()
    assert elay is not None
    ens = K.NormBwdStats(T["enx"], emean, einvstd, T["engamma"], T["enbeta"], 0.2, 2, part("epart", elay[0], 128), elay)
    step("deconv2d_bwd_data.nstats", lambda: K.deconv2d_bwd_data(T["ebdy"], T["ebw"], (8, 8), 2, 2, out=T["ebdx"], nstat=ens))
    step("norm_bwd_partials.batch", lambda: K.norm_lrelu_bwd_from_partials(T["ebdx"], T["enx"], ens, 1))
    assert K.conv_update_form(L.DECONV_BWD_DATA, 2, 8, 8, 128, 16, 16, 64, 5, 5, 2, 2) is not None
    R.close_step()
    step("deconv2d_bwd_data.update", lambda: K.deconv2d_bwd_data(T["ebdy"], T["ebw"], (8, 8), 2, 2, update=K.FusedUpdate(T["etheta"], T["em"], 0.1, 0.0, True)))
    # ---- linear, N > 1 and N = 1
    step("linear_fwd", lambda: K.linear_fwd(T["lx"], T["lw"], T["lb"], L.EPI_LRELU, out=T["ly"]))
    step("linear_fwd.n1", lambda: K.linear_fwd(T["lx"], T["lw1"], T["lb1"]))
    step("linear_bwd_data", lambda: K.linear_bwd_data(T["ly"], T["lw"], out=T["ldx"]))
    step("linear_bwd_data.n1", lambda: K.linear_bwd_data(T["ly1"], T["lw1"]))
    step("linear_out1_bce", lambda: K.linear_out1_bce(T["lx"], T["lw1"], T["lb1"], T["ly1"], T["ldl"], T["llm"]))
    # ---- batch norm, synchronised batch norm, instance norm
    step("bn_bwd", lambda: K.bn_train_lrelu_bwd_data(T["ebdx"], T["enx"], T["engamma"], T["enbeta"], emean, einvstd))
    step("bn_param_grads", lambda: K.bn_train_param_grads(T["enx"], T["edgamma"], T["edbeta"], True))
    sums = T["sums"]
    step("bn_sync_fwd_sums", lambda: K.bn_sync_fwd_sums(T["nx"], sums))
    _, smean, sinvstd = step("bn_sync_fwd_apply", lambda: K.bn_sync_fwd_apply(T["nx"], T["ngamma"], T["nbeta"], sums, 128))
    step("bn_sync_bwd_sums", lambda: K.bn_sync_bwd_sums(T["baux"], T["nx"], T["ngamma"], T["nbeta"], smean, sinvstd, sums))
    step("bn_sync_bwd_apply", lambda: K.bn_sync_bwd_apply(T["baux"], T["nx"], T["ngamma"], T["nbeta"], smean, sinvstd, sums, 128))
    step("instnorm_bwd", lambda: K.instnorm_lrelu_bwd_data(T["baux"], T["nx"], T["ngamma"], T["nbeta"], mean, invstd, 0.2))
    step("instnorm_param_grads", lambda: K.instnorm_param_grads(T["nx"], T["dgamma"], T["dbeta"]))
    # ---- element-wise
    step("add", lambda: K.add(T["cy"], T["nx"]))
    step("bn_fold", lambda: K.bn_fold(T["ngamma"], T["nbeta"], T["mmean"], T["mvar"]))
    step("affine_relu_fwd", lambda: K.affine_relu_fwd(T["cy"], T["ca"], T["cc"]))
    step("affine_relu_bwd", lambda: K.affine_relu_bwd(T["nx"], T["cy"], T["ca"]))
    step("affine_fwd", lambda: K.affine_fwd(T["cy"], T["ca"], T["cc"]))
    step("affine_bwd", lambda: K.affine_bwd(T["cy"], T["ca"]))
    step("lrelu_fwd", lambda: K.lrelu_fwd(T["cy"]))
    step("lrelu_bwd", lambda: K.lrelu_bwd(T["nx"], T["cy"], 0.1))
    step("tanh_fwd", lambda: K.tanh_fwd(T["cy"]))
    step("tanh_bwd", lambda: K.tanh_bwd(T["nx"], T["cy"]))
    # ---- refinement-loop scalars
    step("bce_ones_grad_rowmean", lambda: K.bce_ones_grad_rowmean(T["logits"]))
    step("bce_ones_fwd", lambda: K.bce_ones_fwd(T["logits"]))
    step("bce_ones_bwd", lambda: K.bce_ones_bwd(T["dlogits"], T["logits"]))
    step("sigmoid_rowmean", lambda: K.sigmoid_rowmean(T["logits"]))
    step("clip", lambda: K.clip(T["rtheta"], -0.5, 0.5))
    step("refine_update", lambda: K.refine_update(T["rtheta"], T["rm"], T["rg"], 0.1, 0.9, False, -1.0, 1.0))
    step("refine_select_rows", lambda: K.refine_select_rows(T["rrows"], T["rlogit"], T["rforced"], 1, T["rbrows"], T["rblogit"]))
    step("refine_select", lambda: K.refine_select(T["rtheta"], T["rlogit"], T["rforced"], 1, T["rbest"], T["rblogit"], T["rbstep"]))
    step("refine_select2", lambda: K.refine_select2(T["rrows"], T["rbrows"], T["rtheta"], T["rbest"], T["rlogit"], T["rforced"], 2, T["rblogit"], T["rbstep"], T["tickets"]))
    ladam = T.get("ladam")
    if ladam is None:
        ladam = T["ladam"] = K.LadamState(5, T["cx"].device)
        for name in ("s_real", "loss_avg", "gain"):
            R.add(f"ladam.{name}", getattr(ladam, name))
    ladam.set_real(0.7)
    step("refine_loss_seed", lambda: K.refine_loss_seed(T["logits"], "lsq", ladam=ladam, first=True))
    step("refine_loss_seed.plain", lambda: K.refine_loss_seed(T["logits"], "linear", T["dlogits"], T["lmean"]))
    step("linear_out1_seed", lambda: K.linear_out1_seed(T["lx"], T["lw1"], T["lb1"], T["ly1"], T["ldl"], T["llm"], "bce", ladam, False))
    step("ladam_gain", lambda: K.ladam_gain(T["loss"], T["loss_avg"], T["gain"], True))
    step("refine_update_ladam", lambda: K.refine_update_ladam(T["rtheta"], T["rm"], T["rv"], T["rg"], T["gain"], 0.05, False))
    # ---- weight gradients, losses, Adam
    step("conv2d_bwd_weight", lambda: K.conv2d_bwd_weight(T["cx"], T["cy"], 3, 3, 1, 1, out=T["gdw"], accumulate=True))
    assert K.conv_wgrad_cout1_ok((2, 8, 8, 64), 4, 4, 1, 1)
    R.close_step()
    step("conv2d_bwd_weight_cout1", lambda: K.conv2d_bwd_weight_cout1(T["g1x"], T["g1dy"], 4, 4, 1, 1, out=T["g1dw"]))
    step("deconv2d_bwd_weight", lambda: K.deconv2d_bwd_weight(T["dx"], T["dy"], 3, 3, 2, 2, out=T["gdeconv"]))
    step("linear_bwd_weight", lambda: K.linear_bwd_weight(T["lx"], T["ly"], out=T["glin"]))
    step("bias_grad", lambda: K.bias_grad(T["cy"], out=T["gbias"], accumulate=True))
    step("bce_logits_grad", lambda: K.bce_logits_grad(T["logits"], 1.0, 0.5, loss=T["loss1"]))
    step("gan_logits_grad", lambda: K.gan_logits_grad(T["logits"], "hinge", 0.0, 0.25, T["dlogits"], T["loss1"]))
    step("gan_loss", lambda: K.gan_loss(T["logits"], "lsq", 1.0, dloss=T["dlogits"]))
    step("adam_step", lambda: K.adam_step(T["aw2"], T["ag2"], T["am2"], T["av2"], 1e-3, 0.5, 0.999, 1e-8))
    table = T.get("adam")
    if table is None:
        table = T["adam"] = K.AdamTable([(T["aw"], T["ag"], T["am"], T["av"]), (T["aw2"], T["ag2"], T["am2"], T["av2"])])
        for name in ("table", "plan", "lr_t"):
            R.add(f"adam.{name}", getattr(table, name))
    step("adam_multi", lambda: table.step(1e-3, 0.5, 0.999, 1e-8))
    step("bn_moving_update", lambda: K.bn_moving_update(mean[0], invstd[0], T["mmean"], T["mvar"], 0.9))
    # ---- float64 state: pool moments, Frechet, calibration, modes, density
    for name in ("psum", "pgram", "qsum", "qgram"):
        T[name].zero_()
    step("pool_moments", lambda: K.pool_moments(T["px"], T["psum"], T["pgram"]))
    step("pool_moments.rows", lambda: K.pool_moments(T["px"], T["qsum"], T["qgram"], shift=T["pshift"], rows=np.arange(63, 3, -2)))
    step("spatial_mean", lambda: K.spatial_mean(T["cy"]))
    step("f64_matmul", lambda: K.f64_matmul(T["fa"], T["fb"], out=T["fo"], alpha=0.5, diag=2.0))
    step("frechet", lambda: K.frechet_from_moments(T["psum"], T["pgram"], None, 64, T["qsum"], T["qgram"], T["pshift"], 30, max_iters=6,
                                                   out=T["fd"]))
    step("calibration", lambda: K.calibration_accumulate(T["score"], 1, T["edges"], T["cal"]))
    step("mode_stats", lambda: K.mode_stats_accumulate(T["x2"], T["cent"], 0.3, T["modes"]))
    step("kde2d", lambda: K.kde2d_accumulate(T["x2"], T["axx"], T["axy"], T["whiten"], T["kde"]))
    # ---- rejection sampling, Metropolis-Hastings
    step("drs_set_max", lambda: K.drs_set_max(T["score"], T["drs"]))
    step("drs_decide", lambda: K.drs_decide(T["score"], T["unif"], T["drs"], groups=3, shift_percent=60.0, want_p=True, want_bounds=True))
    step("drs_decide.plain", lambda: K.drs_decide(T["score"], T["unif"], T["drs"], shift_percent=None))
    step("compact_rows", lambda: K.compact_rows(T["rowsrc"], T["mask"], T["pool"], 2))
    step("compact_rows.take_all", lambda: K.compact_rows(T["rowsrc"], T["mask"], T["pool"], 0, take_all=T["takeall"], total=T["total"]))
    step("mh_walk", lambda: K.mh_walk(T["score"], T["unif"], T["mh"], 3))
    T["fill"].zero_()
    rows, _, span = step("mh_walk.fill", lambda: K.mh_walk(T["score"], T["unif"], T["mh"], 3, 1, groups=3, take_all=T["takeall"], fill=T["fill"], capacity=20))
    step("gather_rows", lambda: K.gather_rows(T["rowsrc"], rows, span, T["pool"]))


def profile_summary(profile):
    return {k: [v[0], len(v[1]), v[2], v[3]] for k, v in sorted(profile.items())}


def trace():
    """{"plain": records, "profiled": records, "profile": {...}, "profile_by_layer": {...}} of the script in THIS process."""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import torch
    from cgs_amd import kernels as K, lib as L
    dev = torch.device("cuda:0")
    R = Recorder(L.load(), L.SIGNATURES)
    L._lib = R
    try:
        T = _tensors(R, dev)
        out = {}
        for name, profile, by_layer in (("plain", None, False), ("profiled", {}, False), ("by_layer", {}, True)):
            R.records = []
            K.PROFILE, K.PROFILE_BY_LAYER = profile, by_layer
            try:
                _script(K, L, R, T)
                torch.cuda.synchronize()
            finally:
                K.PROFILE, K.PROFILE_BY_LAYER = None, False
            if name != "by_layer":
                out[name] = R.records
            if profile is not None:
                out["profile" if name == "profiled" else "profile_by_layer"] = profile_summary(profile)
    finally:
        L._lib = R._real
    return json.loads(json.dumps(out))


def dump(tr, path):
    """One record per line: a golden that diffs."""
    with open(path, "w") as f:
        f.write("{\n")
        for name in ("plain", "profiled"):
            f.write(f' "{name}": [\n' + ",\n".join("  " + json.dumps(r) for r in tr[name]) + "\n ],\n")
        for i, name in enumerate(("profile", "profile_by_layer")):
            f.write(f' "{name}": {{\n' + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in tr[name].items()) + "\n }" + (",\n" if i == 0 else "\n"))
        f.write("}\n")


if __name__ == "__main__":
    dump(trace(), sys.argv[1])
