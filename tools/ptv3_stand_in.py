"""A small PointTransformerV3 written from the behaviour of models/pt_v3.py's classes, for the tools and tests that need a
whole backbone pass and have no caller's models/pt_v3.py at hand: tools/seam_bench.py's whole-model item and
tests/test_point_seam_gpu.py.  It is a namespace the installs (point_pool, point_front, point_mid, point_ffn, point_seam,
point_attention) accept in place of the imported module: Point, PointModule, PointSequential, Block, SerializedAttention,
SerializedPooling, SerializedUnpooling, Embedding, PointTransformerV3 and a spconv namespace.

What stands in: the sparse convolutions are a bias-free Linear on the sparse tensor's features (`Conv`); serialization is
a z-order code in torch ops ("z": x, y, z; any other name: y, x, z) with the batch above 3 * depth bits; the attention is
the non-flash branch; pooling takes upstream's steps in torch ops with stable sorts (`max` for the features, the mean of
coord).  Everything runs on the CPU in float64 as well as on the GPU.  sloped_frame() is tools/point_pool_bench.py's frame.
"""
import math
import types

import numpy as np
import torch


class Sparse:
    """spconv.SparseConvTensor by what the backbone reads of it: features and replace_feature."""
    def __init__(self, features):
        self.features = features

    def replace_feature(self, features):
        return Sparse(features)


class Point(dict):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if "offset" not in self and "batch" in self:
            self["offset"] = torch.cumsum(torch.bincount(self["batch"]), 0)

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        self[k] = v

    def serialization(self, order="z", depth=None, shuffle_orders=False):
        names = [order] if isinstance(order, str) else list(order)
        if depth is None:
            depth = int(self.grid_coord.max()).bit_length()
        g = self.grid_coord.long()
        codes = []
        for name in names:
            a, b, c = (g[:, 0], g[:, 1], g[:, 2]) if name == "z" else (g[:, 1], g[:, 0], g[:, 2])
            code = torch.zeros_like(a)
            for i in range(depth):
                code |= (((a >> i) & 1) << (3 * i + 2)) | (((b >> i) & 1) << (3 * i + 1)) | (((c >> i) & 1) << (3 * i))
            codes.append(code | (self.batch.long() << (3 * depth)))
        code = torch.stack(codes)
        order_ = torch.sort(code, dim=1, stable=True).indices
        inverse = torch.zeros_like(order_).scatter_(1, order_, torch.arange(code.shape[1], device=code.device).repeat(len(names), 1))
        self["serialized_depth"], self["serialized_code"] = depth, code
        self["serialized_order"], self["serialized_inverse"] = order_, inverse

    def sparsify(self, pad=96):
        self["sparse_conv_feat"] = Sparse(self.feat)


class PointModule(torch.nn.Module):
    pass


class Conv(torch.nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.lin = torch.nn.Linear(cin, cout, bias=False)

    def forward(self, s):
        return s.replace_feature(self.lin(s.features))


spconv = types.SimpleNamespace(modules=types.SimpleNamespace(is_spconv_module=lambda m: isinstance(m, Conv)))


class PointSequential(PointModule):
    def __init__(self, *mods):
        super().__init__()
        for m in mods:
            self.add(m)

    def add(self, module):
        self.add_module(str(len(self._modules)), module)

    def forward(self, x):
        for module in self._modules.values():
            if isinstance(module, PointModule):
                x = module(x)
            elif spconv.modules.is_spconv_module(module):
                x.sparse_conv_feat = module(x.sparse_conv_feat)
                x.feat = x.sparse_conv_feat.features
            elif isinstance(module, torch.nn.BatchNorm1d):
                if x.feat.size(0) != 1:
                    x.feat = module(x.feat)
            else:
                x.feat = module(x.feat)
                if "sparse_conv_feat" in x.keys():
                    x.sparse_conv_feat = x.sparse_conv_feat.replace_feature(x.feat)
        return x


class MLP(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.fc1, self.act, self.fc2 = torch.nn.Linear(c, 4 * c), torch.nn.GELU(), torch.nn.Linear(4 * c, c)

    def forward(self, x):
        return self.fc2(self.act(self.fc1(x)))


class SerializedAttention(PointModule):
    """The non-flash branch: patches of K = min(smallest batch element, patch_size_max) points in serialized order, a batch
    element's last patch filled up from the one before."""
    def __init__(self, channels, num_heads, patch_size, order_index=0):
        super().__init__()
        self.channels, self.num_heads, self.scale, self.order_index = channels, num_heads, (channels // num_heads) ** -0.5, order_index
        self.enable_flash = self.enable_rpe = False
        self.patch_size_max, self.patch_size = patch_size, 0
        self.attn_drop, self.proj_drop = torch.nn.Dropout(0.0), torch.nn.Dropout(0.0)
        self.qkv, self.proj = torch.nn.Linear(channels, channels * 3), torch.nn.Linear(channels, channels)

    def get_padding_and_inverse(self, point):
        K, pad, unpad, cu, start, pstart = self.patch_size, [], [], [torch.zeros(1, dtype=torch.int64)], 0, 0
        for end in point.offset.tolist():
            n = end - start
            own = [torch.arange(n)]
            if n > K and n % K:
                m, r = n // K, n % K
                own.append(torch.arange((m - 1) * K + r, m * K))
            own = torch.cat(own)
            pad.append(start + own)
            unpad.append(pstart + torch.arange(n))
            cu.append(pstart + torch.arange(K, len(own) + 1, K) if n >= K else torch.tensor([pstart + n]))
            start, pstart = end, pstart + len(own)
        dev = point.offset.device
        return torch.cat(pad).to(dev), torch.cat(unpad).to(dev), torch.cat(cu).to(dev, torch.int32)

    def forward(self, point):
        counts = torch.diff(point.offset, prepend=point.offset.new_zeros(1))
        self.patch_size = K = min(int(counts.min()), self.patch_size_max)
        H, C = self.num_heads, self.channels
        pad, unpad, _ = self.get_padding_and_inverse(point)
        order = point.serialized_order[self.order_index][pad]
        inverse = unpad[point.serialized_inverse[self.order_index]]
        q, k, v = self.qkv(point.feat)[order].reshape(-1, K, 3, H, C // H).permute(2, 0, 3, 1, 4).unbind(dim=0)
        attn = torch.softmax((q * self.scale) @ k.transpose(-2, -1), dim=-1)
        feat = (attn @ v).transpose(1, 2).reshape(-1, C)[inverse]
        point.feat = self.proj_drop(self.proj(feat))
        return point


class Block(PointModule):
    """pre_norm: the order of its modules and of its residual adds."""
    def __init__(self, c, patch_size, order_index=0):
        super().__init__()
        self.pre_norm = True
        self.cpe = PointSequential(Conv(c, c), torch.nn.Linear(c, c), torch.nn.LayerNorm(c))
        self.norm1 = PointSequential(torch.nn.LayerNorm(c))
        self.attn = SerializedAttention(c, c // 16, patch_size, order_index)
        self.norm2, self.mlp = PointSequential(torch.nn.LayerNorm(c)), PointSequential(MLP(c))
        self.drop_path = PointSequential(torch.nn.Identity())

    def forward(self, point):
        shortcut = point.feat
        point = self.cpe(point)
        point.feat = shortcut + point.feat
        shortcut = point.feat
        point = self.norm1(point)
        point = self.drop_path(self.attn(point))
        point.feat = shortcut + point.feat
        shortcut = point.feat
        point = self.norm2(point)
        point = self.drop_path(self.mlp(point))
        point.feat = shortcut + point.feat
        point.sparse_conv_feat = point.sparse_conv_feat.replace_feature(point.feat)
        return point


class SerializedPooling(PointModule):
    def __init__(self, cin, cout, stride, norm_layer, act_layer, reduce="max", shuffle_orders=False, traceable=True):
        super().__init__()
        self.stride, self.reduce, self.shuffle_orders, self.traceable = stride, reduce, shuffle_orders, traceable
        self.proj = torch.nn.Linear(cin, cout)
        self.norm, self.act = PointSequential(norm_layer(cout)), PointSequential(act_layer())

    def forward(self, point):
        depth = (math.ceil(self.stride) - 1).bit_length()
        if depth > point.serialized_depth:
            depth = 0
        code = point.serialized_code >> depth * 3
        _, cluster, counts = torch.unique(code[0], sorted=True, return_inverse=True, return_counts=True)
        indices = torch.sort(cluster, stable=True).indices
        idx_ptr = torch.cat([counts.new_zeros(1), torch.cumsum(counts, dim=0)])
        head = indices[idx_ptr[:-1]]
        code = code[:, head]
        order = torch.sort(code, dim=1, stable=True).indices
        inverse = torch.zeros_like(order).scatter_(1, order, torch.arange(code.shape[1], device=code.device).repeat(code.shape[0], 1))
        feat, s = self.proj(point.feat), counts.shape[0]
        pooled = feat.new_full((s, feat.shape[1]), float("-inf")).scatter_reduce(0, cluster[:, None].expand(-1, feat.shape[1]), feat, "amax")
        coord = point.coord.new_zeros((s, 3)).index_add_(0, cluster, point.coord) / counts[:, None].to(point.coord.dtype)
        out = Point(feat=pooled, coord=coord, grid_coord=point.grid_coord[head] >> depth, serialized_code=code,
                    serialized_order=order, serialized_inverse=inverse, serialized_depth=point.serialized_depth - depth,
                    batch=point.batch[head])
        if self.traceable:
            out["pooling_inverse"], out["pooling_parent"] = cluster, point
        if self.norm is not None and out.feat.size(0) != 1:
            out = self.norm(out)
        if self.act is not None:
            out = self.act(out)
        out.sparsify()
        return out


class SerializedUnpooling(PointModule):
    def __init__(self, cin, cskip, cout, norm_layer, act_layer, traceable=False):
        super().__init__()
        self.proj = PointSequential(torch.nn.Linear(cin, cout), norm_layer(cout), act_layer())
        self.proj_skip = PointSequential(torch.nn.Linear(cskip, cout), norm_layer(cout), act_layer())
        self.traceable = traceable

    def forward(self, point):
        parent, inverse = point.pop("pooling_parent"), point.pop("pooling_inverse")
        point, parent = self.proj(point), self.proj_skip(parent)
        parent.feat = parent.feat + point.feat[inverse]
        return parent


class Embedding(PointModule):
    def __init__(self, cin, cout, norm_layer, act_layer):
        super().__init__()
        self.stem = PointSequential(Conv(cin, cout), norm_layer(cout), act_layer())

    def forward(self, point):
        return self.stem(point)


class PointTransformerV3(PointModule):
    """Encoder stages of `widths` (a pooling in front of every stage but the first), then the decoder back up."""
    def __init__(self, cin=6, widths=(32, 64), orders=("z", "z-trans"), patch_size=48, depth=None):
        super().__init__()
        bn = lambda c: torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.01)  # noqa: E731
        self.orders, self.depth = list(orders), depth
        self.embedding = Embedding(cin, widths[0], bn, torch.nn.GELU)
        self.enc, self.dec = PointSequential(), PointSequential()
        for s, c in enumerate(widths):
            stage = PointSequential()
            if s:
                stage.add(SerializedPooling(widths[s - 1], c, 2, bn, torch.nn.GELU))
            stage.add(Block(c, patch_size, s % len(self.orders)))
            self.enc.add(stage)
        dec, cur = [widths[min(1, len(widths) - 1)]] + list(widths[1:-1]), widths[-1]   # (64, 64, 128, 256) for config.py's widths
        for s in reversed(range(len(widths) - 1)):
            stage = PointSequential(SerializedUnpooling(cur, widths[s], dec[s], bn, torch.nn.GELU))
            stage.add(Block(dec[s], patch_size, s % len(self.orders)))
            self.dec.add(stage)
            cur = dec[s]

    def forward(self, data):
        point = Point(data)
        point.serialization(order=self.orders, depth=self.depth)
        point.sparsify()
        return self.dec(self.enc(self.embedding(point)))


NAMESPACE = types.SimpleNamespace(Point=Point, PointModule=PointModule, PointSequential=PointSequential, Block=Block,
                                  SerializedAttention=SerializedAttention, SerializedPooling=SerializedPooling,
                                  SerializedUnpooling=SerializedUnpooling, Embedding=Embedding,
                                  PointTransformerV3=PointTransformerV3, spconv=spconv)


def sloped_frame(points, batches, depth, cin=6, seed=None):
    """tools/point_pool_bench.py's frame: every batch element a sloped surface three voxels thick inside a box of 48 x 48
    columns.  Returns host tensors: feat [n, cin], coord, grid_coord int32, batch."""
    rng = np.random.default_rng(points if seed is None else seed)
    counts = rng.multinomial(points - batches, np.ones(batches) / batches) + 1
    batch = np.repeat(np.arange(batches), counts)
    origin = np.repeat(rng.integers(0, (1 << depth) - 48, (batches, 2)), counts, axis=0)
    xy = origin + rng.integers(0, 48, (points, 2))
    z = ((xy[:, 0] + xy[:, 1]) // 4 + rng.integers(0, 3, points)) & ((1 << depth) - 1)
    grid = np.concatenate([xy, z[:, None]], 1).astype(np.int32)
    return {"feat": torch.from_numpy(rng.standard_normal((points, cin)).astype(np.float32)),
            "coord": torch.from_numpy(grid.astype(np.float32) * 0.01), "grid_coord": torch.from_numpy(grid),
            "batch": torch.from_numpy(batch.astype(np.int64))}
