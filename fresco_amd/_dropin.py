"""What the drop-ins for the UNet's modules share (unet_resnet, unet_transformer, unet_attention):
finding a model's modules by their parts, the refusal sentence, binding and unbinding `forward`, the state-dict intake, and
the layout rules at a drop-in's boundary.  Nothing here launches a kernel or knows a module's arithmetic."""
import torch


def f32(t, device):
    return t.detach().to(device, torch.float32).contiguous()


def find(model, parts):
    """[(name, module)] of the modules of `model` that have every attribute in `parts`"""
    return [(name, m) for name, m in model.named_modules() if all(hasattr(m, p) for p in parts)]


def refusal(who, name, why):
    """the NotImplementedError for a module `name` outside what `who` computes; name "": what a call itself does not take"""
    return NotImplementedError("%s: %s; there is no fallback to PyTorch" % (who, (name + " " + why).lstrip()))


DTYPE_NAMES = {torch.float16: "fp16", torch.bfloat16: "bf16"}


def dtype_name(who, dtype):
    """"fp16" / "bf16" for a drop-in's `dtype` argument (the pipeline's torch_dtype); anything else is refused"""
    if dtype not in DTYPE_NAMES:
        raise TypeError("%s: dtype must be torch.float16 or torch.bfloat16, got %s" % (who, dtype))
    return DTYPE_NAMES[dtype]


def check_all(who, found, cls, dtype=torch.float16):
    """refuse, by name, the first of `found` that cls.refusal objects to: call it before anything is patched"""
    for name, m in found:
        why = cls.refusal(m) if dtype == torch.float16 else cls.refusal(m, dtype=dtype)
        if why:
            raise refusal(who, name or "the model", why)


def patch(model, cls, parts, who, attr, memory_format, dtype=torch.float16):
    """bind cls.from_module(m) as `forward` (and under `attr`) in the __dict__ of every module of `model` that has `parts`;
    every module is checked first.  The modules' own methods stay on their class.  dtype: the pipeline's dtype; a drop-in
    that has no bf16 form is not handed the argument (the default).  -> the number of modules patched"""
    check_format(who, memory_format)
    extra = {} if dtype == torch.float16 else {"dtype": dtype}
    unpatch(model, attr)
    found = find(model, parts)
    check_all(who, found, cls, dtype)
    for name, m in found:
        native = cls.from_module(m, memory_format=memory_format, name=name, **extra)
        m.__dict__[attr] = native
        m.__dict__["forward"] = native
    return len(found)


def unpatch(model, attr):
    """remove what patch bound under `attr`; -> the number of modules restored"""
    count = 0
    for _, m in model.named_modules():
        if attr in vars(m):
            del m.__dict__[attr]
            m.__dict__.pop("forward", None)
            count += 1
    return count


def intake(state_dict, prefix, need, who, default, dtype=torch.float16):
    """the entries of `state_dict` under `prefix`, without it -> (sd, what), `what` the prefix of the caller's messages
    ("<who>: <prefix, or `default`>").  Every name in `need` must be there (the first four missing ones are reported) and
    of `dtype` (fp16 unless the caller has a bf16 form).  Entries that `need` does not name are kept as they are: check_shapes
    decides about them."""
    if prefix and not prefix.endswith("."):
        prefix += "."
    sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
    what = "%s: %s" % (who, prefix[:-1] or default)
    missing = [k for k in need if k not in sd]
    if missing:
        raise ValueError("%s: missing parameters %s" % (what, missing[:4]))
    for k in need:
        if sd[k].dtype != dtype:
            if dtype == torch.float16:
                raise TypeError("%s: fp16 parameters only (%s is %s); bf16 and fp32 UNets are not supported" % (what, k, sd[k].dtype))
            raise TypeError("%s: %s parameters only with dtype=%s (%s is %s)" % (what, DTYPE_NAMES[dtype], dtype, k, sd[k].dtype))
    return sd, what


def check_shapes(sd, shapes, what, only):
    """every entry of the {name: shape} table must be in `sd` with that shape.  With `only` (the resnet) an entry the table
    does not name is refused as unexpected; without (the transformer) it is ignored: the attention modules' own weights sit
    under the same prefix and belong to those modules."""
    for k, shp in shapes.items():
        got = tuple(sd[k].shape) if k in sd else None
        if got != shp:
            raise ValueError("%s: %s is %s, expected %s" % (what, k, got, shp))
    extra = sorted(k for k in sd if k not in shapes) if only else None
    if extra:
        raise ValueError("%s: unexpected parameters %s" % (what, extra[:4]))


def check_format(who, memory_format):
    if memory_format not in (torch.channels_last, torch.contiguous_format):
        raise ValueError("%s: memory_format must be channels_last or contiguous_format" % who)


def rows16(x):
    """x as dense rows at a 16-byte aligned address: itself where it is that already, otherwise one copy"""
    if not x.is_contiguous():
        return x.contiguous()
    return x.clone() if x.data_ptr() % 16 else x


def nhwc(x):
    """logical NCHW -> (n, H, W, C) in memory: a view of a channels_last tensor, a copy of any other"""
    return rows16(x.permute(0, 2, 3, 1))


def nchw(out, memory_format):
    """(n, H, W, C) -> logical NCHW: channels_last as it is, contiguous_format by one copy (check_format has passed)"""
    out = out.permute(0, 3, 1, 2)
    return out if memory_format == torch.channels_last else out.contiguous()
