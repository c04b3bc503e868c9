'''
fc_layers — the reference's fully-connected call-site modules on the MI355X kernels.

`cublasLinear` and `cusparseLinear` keep the constructor, parameters, initialisation and
`forward(inp)` contract of the reference's modules (benchmarks/cublas_fc_layer.py:12-51,
benchmarks/cusparse_fc_layer.py:12-51): `y = inp @ weight.t() + bias` with `weight`
`[out_features, in_features]`, any number of leading dims on `inp`.

The reference computes `t = cublasMM.apply(inp, self.weight.t()); output = t.clone();
output += self.bias` — a product, a copy and an add, i.e. two extra passes over the output.
Here the bias is added in the kernel epilogue (`custom_mm.cublas_mmul_bias` /
`custom_mm.naive_spmm_bias`) and the backward runs on the same
kernels: grad_inp = dY·W, grad_W = dYᵀ·inp, grad_bias = 1ᵀ·dY.

`cusparseLinear` treats the *activations* as the sparse operand, exactly like the reference
(`cusparseMM.apply(inp, weight.t())`: exact zeros of `inp` are dropped, e.g. after a ReLU).

bfloat16 / float16: a layer moved with `.to(torch.bfloat16)` takes inputs of that dtype and
returns it, forward and backward — the product on the matrix cores with the bias in its epilogue, the weight
gradient through the deterministic split-k (`custom_mm.cublas_mmul_splitk`), the bias gradient by
`custom_mm.column_sums`; fp32 sums, each element rounded once.  The input and the parameters must share one dtype.

`blockSparseLinear` (an addition) is the layer with a block-pruned WEIGHT: the kept 64 × 64 blocks of
`weight` are its parameter, the layout a pair of buffers; bfloat16 / float16 only (`matmuls.block_sparse_linear`).
'''

import math

import torch
import torch.nn as nn
from torch.autograd.function import InplaceFunction

import custom_mm
from matmuls import block_sparse_linear, custom_matmul, sampled_density


def _column_sums(g2d):
    '''Bias gradient: column sums of dY on the device (custom_mm.column_sums).'''
    return custom_mm.column_sums(g2d)


_LOWP = (torch.bfloat16, torch.float16)


def _check_dtypes(inp, weight, bias):
    '''One dtype for the input and the parameters, named before anything runs (the rule of custom_matmul).'''
    for name, p in (('weight', weight), ('bias', bias)):
        if p is not None and p.dtype != inp.dtype:
            raise RuntimeError('fc_layers: the input is {} but the layer\'s {} is {}: convert one of them '
                               '(layer.to(dtype) or input.to(dtype))'.format(inp.dtype, name, p.dtype))


def _dense_forward(x2, weight, bias, out):
    if bias is not None:
        custom_mm.cublas_mmul_bias(x2, weight, bias, out, False, True)
    else:
        custom_mm.cublas_mmul(x2, weight, out, False, True)


def _weight_grad(g2, x2):
    '''dYᵀ·x.  bfloat16 / float16: a long k (the tokens) over few output tiles — the deterministic split-k; a shape the
    rule does not split gets the plain product's bits by construction.'''
    if g2.dtype in _LOWP:
        gw = torch.empty((g2.shape[1], x2.shape[1]), device=g2.device, dtype=g2.dtype)
        return custom_mm.cublas_mmul_splitk(g2, x2, gw, True, False)
    return custom_matmul(g2, x2, transa=True)


class _LinearBias(InplaceFunction):
    '''y = x·Wᵀ (+ bias) with the dense kernel; x [..., in], W [out, in].'''

    @staticmethod
    def forward(ctx, inp, weight, bias):
        _check_dtypes(inp, weight, bias)
        ctx.save_for_backward(inp, weight)
        ctx.has_bias = bias is not None
        x2 = inp.reshape(-1, inp.shape[-1])
        out = torch.empty((x2.shape[0], weight.shape[0]), device=inp.device, dtype=inp.dtype)
        _dense_forward(x2, weight, bias, out)
        return out.view(tuple(inp.shape[:-1]) + (weight.shape[0],))

    @staticmethod
    def backward(ctx, grad_output):
        inp, weight = ctx.saved_tensors
        g2 = grad_output.reshape(-1, grad_output.shape[-1])
        x2 = inp.reshape(-1, inp.shape[-1])
        grad_inp = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            grad_inp = custom_matmul(g2, weight).view(inp.shape)       # dY·W
        if ctx.needs_input_grad[1]:
            grad_w = _weight_grad(g2, x2)                               # dYᵀ·x
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_b = _column_sums(g2)
        return grad_inp, grad_w, grad_b


def sparse_forward_pays(nnz, tokens, in_features, out_features):
    '''Forward cost model of `cusparseLinear` (fitted on MI355X, tools/bench_fc.py,
    profiles/r02_fc_layer_timings.log): the exact-fp32 MFMA product runs at ≈130 TFLOP/s on these
    shapes, the row-split SpMM of ReLU-sparse activations at ≈15 TFLOP/s of useful flops, plus three
    passes over the activations for the exact count and the fill.  Sparse is taken only when the
    model gives it a 10 % lead.'''
    t_dense = 2.0 * tokens * in_features * out_features / 130e12
    t_sparse = 2.0 * nnz * out_features / 15e12 + 3.0 * tokens * in_features * 4 / 4e12
    return t_sparse < 0.9 * t_dense


_SAMPLE_ROWS = 512


def worth_sampling(tokens, in_features, out_features):
    '''A layer whose dense product takes under a quarter of a millisecond cannot win back the sample's
    launches + read-back (≈0.03 ms): measured 0.232 vs 0.200 ms at 16384 × 3072 → 256.'''
    return 2.0 * tokens * in_features * out_features / 130e12 >= 0.25e-3


class _SparseLinearBias(InplaceFunction):
    '''y = sparse(x)·Wᵀ (+ bias): the activations' exact zeros are skipped when that pays.

    The layer first estimates the density from an evenly spaced sample of ≤ 512 token rows (one small
    count kernel).  Since round 4 the count comes back WITHOUT stalling the stream (matmuls.sampled_density:
    pinned memory behind an event; a forward decides from the most recent count that has landed for this
    layer's shapes — the previous step's, in a loop — so only the first forward of a shape waits; the
    reference's cusparseDenseToSparse analysis step synchronises on every call, src/baseline_mm.cu:232-247).
    When the model says the sparse route wins, the conversion needs no read-back either where the layer is no
    wider than the long-row threshold: the CSR arrays get room for every element of x (the fill cannot
    overflow) and the kernels walk the rows through the offsets; the estimate only steers their choice of
    plan.  Otherwise the dense MFMA product runs.  Both routes sum the same terms in the same (column)
    order, the skipped ones being exact zeros, so the result does not depend on the route (finite weights;
    a zero of x facing an inf / nan weight gives nan on the dense route, as in torch.matmul).  Under stream
    capture nothing may be read back: the dense product is used.  (The fused zero-skipping kernel of naiveSpMM is not
    used here: it scans every element of x per 64 output columns and lost to both routes at FC sizes —
    0.46 ms vs 0.20 ms dense at 16384 × 3072 → 256, 99 % zeros.)'''

    @staticmethod
    def forward(ctx, inp, weight, bias):
        _check_dtypes(inp, weight, bias)
        ctx.has_bias = bias is not None
        x2 = inp.reshape(-1, inp.shape[-1])
        tokens, fin, fout = x2.shape[0], x2.shape[1], weight.shape[0]
        out = torch.empty((tokens, fout), device=inp.device, dtype=inp.dtype)
        csr = None
        capturing = inp.is_cuda and torch.cuda.is_current_stream_capturing()
        ctx.x_density = 1.0
        nnz_arg = 0
        ctx.exact_csr = True
        lowp = inp.dtype in _LOWP  # always the dense route: no sample, no conversion (class docstring of cusparseLinear)
        if not lowp and not capturing and x2.numel() > 0 and worth_sampling(tokens, fin, fout):
            est = sampled_density(x2, ('fc', tuple(x2.shape), fout, inp.device.index), fin, owner=inp,
                                  sample_rows=_SAMPLE_ROWS)
            ctx.x_density = est
            if sparse_forward_pays(est * x2.numel(), tokens, fin, fout):
                offsets = custom_mm.dense_row_offsets(x2)
                if fin <= custom_mm.long_row_threshold():
                    # no read-back: room for every element.  The count the kernels are told is the estimate — possibly
                    # BELOW the true count (stale or sampled): allowed here because rule 0 runs without the long-row
                    # workspace, the only thing sized from it (include/mi_spmm.h); MI_SPMM_LDS_B takes the clamp of its
                    # 16-byte loads from max(count, offsets' last entry) on the device, every other plan reads through
                    # the offsets alone (tests: test_spmm_count_as_bound_or_estimate_same_bits, test_cusparse_linear_lds_fit_…)
                    values, columns = custom_mm.dense_to_csr_fill(x2, offsets, x2.numel())
                    csr = (values, columns, offsets.view(-1))
                    nnz_arg = min(x2.numel(), max(1, int(est * x2.numel())))
                    ctx.exact_csr = False
                else:
                    nnz = int(offsets.view(-1)[-1])  # wide layers: the long-row rule sizes its lists from the exact count
                    ctx.x_density = nnz / x2.numel()
                    if sparse_forward_pays(nnz, tokens, fin, fout):
                        values, columns = custom_mm.dense_to_csr_fill(x2, offsets, nnz)
                        csr = (values, columns, offsets.view(-1))
                        nnz_arg = nnz
        if csr is not None:
            wt = weight.t().contiguous()                                 # [in, out] row-major B operand
            # rows of x have at most `fin` non-zeros (no duplicate columns): a layer no wider than the long-row
            # threshold runs as ONE launch, without the workspace and the helper kernels of the long-row rule
            rule = 0 if fin <= custom_mm.long_row_threshold() else -1
            if bias is not None:
                custom_mm.naive_spmm_bias_ex(csr[0], csr[1], csr[2], nnz_arg, tokens, fin, wt, bias, out, rule)
            else:
                custom_mm.naive_spmm_ex(csr[0], csr[1], csr[2], nnz_arg, tokens, fin, wt, out, rule)
        else:
            _dense_forward(x2, weight, bias, out)
        ctx.has_csr = csr is not None
        ctx.save_for_backward(inp, weight, *(csr or ()))
        return out.view(tuple(inp.shape[:-1]) + (fout,))

    @staticmethod
    def backward(ctx, grad_output):
        inp, weight = ctx.saved_tensors[:2]
        g2 = grad_output.reshape(-1, grad_output.shape[-1])
        x2 = inp.reshape(-1, inp.shape[-1])
        grad_inp = grad_w = grad_b = None
        if ctx.needs_input_grad[0]:
            grad_inp = custom_matmul(g2, weight).view(inp.shape)       # dense gradient, as torch autograd gives
        if ctx.needs_input_grad[1] and (ctx.x_density > 0.12 or not ctx.has_csr):
            # x is not sparse enough for the sparse route to pay (in × out is a small output: few
            # workgroups): the dense product sums the same terms in the same token order, the
            # skipped ones being exact zeros.  Measured at 16384 tokens, 3072 → 768, half zeros:
            # forward + backward 9.1 → 3.6 ms (tools/bench_fc.py).
            grad_w = _weight_grad(g2, x2)
        elif ctx.needs_input_grad[1]:
            # dYᵀ·x = (xᵀ·dY)ᵀ with x sparse: the CSR kept from forward, transposed, then the row-split kernel
            values, columns, offsets = ctx.saved_tensors[2:]
            # (arrays sized for every element of x: the transpose needs the exact count — the one read-back of this route)
            nnz = values.numel() if ctx.exact_csr else int(offsets[-1])
            t_val, t_col, t_off = custom_mm.csr_transpose(values[:nnz], columns[:nnz], offsets, nnz,
                                                          x2.shape[0], x2.shape[1])
            gwt = torch.empty((x2.shape[1], g2.shape[1]), device=g2.device, dtype=torch.float32)
            custom_mm.naive_spmm(t_val, t_col, t_off, nnz, x2.shape[1], x2.shape[0], g2, gwt)
            grad_w = gwt.t()
        if ctx.has_bias and ctx.needs_input_grad[2]:
            grad_b = _column_sums(g2)
        return grad_inp, grad_w, grad_b


class _LinearBase(nn.Module):
    _fn = None

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        torch.manual_seed(0)  # the reference seeds here (cublas_fc_layer.py:15)

        self.in_features = in_features
        self.out_features = out_features
        self.weight = nn.Parameter(torch.empty(out_features, in_features))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_features))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in, _ = nn.init._calculate_fan_in_and_fan_out(self.weight)
            bound = 1 / math.sqrt(fan_in)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, inp):
        if inp.shape[-1] != self.in_features:
            print('Invalid dimensions')  # reference behaviour (cublas_fc_layer.py:37-40)
            return 0
        return type(self)._fn.apply(inp, self.weight, self.bias)

    def extra_repr(self):
        return 'in_features={}, out_features={}, bias={}'.format(
            self.in_features, self.out_features, self.bias is not None
        )


class cublasLinear(_LinearBase):
    _fn = _LinearBias


class cusparseLinear(_LinearBase):
    '''The layer whose activations' exact zeros are skipped when that pays (float32).

    In bfloat16 / float16 the layer takes the dense route unconditionally — no density sample, no conversion — and so
    returns exactly what `cublasLinear` returns for the same parameters, forward and backward.  In those dtypes the
    two routes would sum in different orders (the MFMA's 32-deep k-steps against the CSR kernels' fmaf chain), so
    "the route never changes the result", which the float32 layer guarantees, could not hold; and a sparse route
    would need a bias epilogue in the low-precision CSR kernels and a 2-byte dense → CSR conversion.'''
    _fn = _SparseLinearBias


def _block_rows(crow):
    '''The block row of every stored entry of a CSR layout.'''
    rows = crow.numel() - 1
    return torch.repeat_interleave(torch.arange(rows, device=crow.device), (crow[1:] - crow[:-1]).to(torch.int64))


def _kept_blocks(weight, crow, col):
    '''[n, 64, 64]: the blocks of a dense [out, in] weight at the stored entries of the layout, in stored-entry order.'''
    out_f, in_f = weight.shape
    blocks = weight.reshape(out_f // 64, 64, in_f // 64, 64).permute(0, 2, 1, 3)
    return blocks[_block_rows(crow), col.to(torch.int64)].contiguous()


class blockSparseLinear(nn.Module):
    '''y = inp @ W.t() + bias with a block-pruned weight: `layout` a 2-d CSR tensor [out_features/64, in_features/64]
    whose stored entries are the kept 64 × 64 blocks of W (matmuls.block_sparse_linear; bfloat16 / float16 — move the layer
    with `.to(device, dtype)`).  Parameters: `values` [n, 64, 64], the kept blocks in stored-entry order, and `bias`; the
    layout's `crow_indices` / `col_indices` are buffers, so they move, save and load with the module.  The CSR layout
    tensor the kernels' sorted and transposed lists live on is rebuilt from the buffers only when they move or are
    overwritten, and kept on the module otherwise.

    Initialisation is `cublasLinear`'s — the same seed, the same kaiming_uniform_ on a dense [out, in] weight, the same
    bias — with the kept blocks taken from that weight: a full layout starts with exactly `cublasLinear`'s parameters.'''

    def __init__(self, in_features, out_features, layout, bias=True):
        super().__init__()
        torch.manual_seed(0)  # as _LinearBase
        if in_features % 64 != 0 or out_features % 64 != 0:
            raise ValueError('blockSparseLinear: in_features and out_features must be multiples of 64, got {} and {}'.format(
                in_features, out_features))
        if not isinstance(layout, torch.Tensor) or layout.layout != torch.sparse_csr or layout.dim() != 2 or \
                tuple(layout.shape) != (out_features // 64, in_features // 64):
            raise ValueError('blockSparseLinear: the layout must be a 2-d CSR tensor [out_features/64, in_features/64] = '
                             '[{}, {}]'.format(out_features // 64, in_features // 64))
        self.in_features = in_features
        self.out_features = out_features
        self.register_buffer('crow_indices', layout.crow_indices().detach().clone())
        self.register_buffer('col_indices', layout.col_indices().detach().clone())
        weight = torch.empty(out_features, in_features)
        nn.init.kaiming_uniform_(weight, a=math.sqrt(5))
        self.values = nn.Parameter(_kept_blocks(weight, self.crow_indices.cpu(), self.col_indices.cpu()))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_features))
            bound = 1 / math.sqrt(in_features)  # fan_in of the dense weight
            nn.init.uniform_(self.bias, -bound, bound)
        else:
            self.register_parameter('bias', None)
        self._layout = self._layout_key = None

    @classmethod
    def from_dense(cls, weight, layout, bias=None):
        '''The layer whose kept blocks are those of the dense `weight` [out, in] (what lies outside the layout is dropped)
        and whose bias is `bias`, in the dtype and on the device of `weight`.'''
        layer = cls(weight.shape[1], weight.shape[0], layout, bias=bias is not None).to(device=weight.device, dtype=weight.dtype)
        with torch.no_grad():
            layer.values.copy_(_kept_blocks(weight.detach(), layer.crow_indices, layer.col_indices))
            if bias is not None:
                layer.bias.copy_(bias.detach())
        return layer

    def layout(self):
        '''The CSR layout tensor [out/64, in/64] on the buffers as they are now (no copy of the indices).'''
        crow, col = self.crow_indices, self.col_indices
        key = (crow.data_ptr(), col.data_ptr(), str(crow.device), crow._version, col._version)
        if self._layout is None or self._layout_key != key:
            marks = torch.ones(col.numel(), dtype=torch.float32, device=col.device)
            self._layout = torch.sparse_csr_tensor(crow, col, marks, size=(self.out_features // 64, self.in_features // 64))
            self._layout_key = key
        return self._layout

    def dense_weight(self):
        '''W [out, in] with zeros outside the layout (differentiable in `values`).'''
        rows, cols = self.out_features // 64, self.in_features // 64
        blocks = self.values.new_zeros((rows, cols, 64, 64))
        blocks = blocks.index_put((_block_rows(self.crow_indices), self.col_indices.to(torch.int64)), self.values)
        return blocks.permute(0, 2, 1, 3).reshape(self.out_features, self.in_features)

    def forward(self, inp):
        if inp.shape[-1] != self.in_features:
            print('Invalid dimensions')  # reference behaviour (cublas_fc_layer.py:37-40)
            return 0
        _check_dtypes(inp, self.values, self.bias)
        return block_sparse_linear(inp, self.values, self.layout(), self.bias)

    def extra_repr(self):
        return 'in_features={}, out_features={}, kept_blocks={} of {}, bias={}'.format(
            self.in_features, self.out_features, self.values.shape[0], (self.in_features // 64) * (self.out_features // 64),
            self.bias is not None)
