"""The tests' model of the bf16 weight layouts (include/snake_env.h
snake_dqn_layout): the packing DQNForward.__init__ did with torch ops until the
library took every forward through snake_dqn_pack32. It lives here, as it
stood, so that "equals the torch packing" compares the pack with a second
definition of the layouts and not with itself. Only the plan and the row table
come from the library (snake_dqn_plan / snake_dqn_rows and their map forms)."""
import ctypes

import torch


def torch_pack(state, plan, h, w, c, A, device='cpu'):
    """The twelve tensors of a bf16 forward (bf16 words as int16, the rest
    float32) for a state dict of the reference's names."""
    from marlenv._native import DqnCfg, DqnLayout, check, lib
    L = lib()
    cfg = DqnCfg(int(h), int(w), int(c), int(A), 0)
    lay = DqnLayout()
    plan_fn, rows_fn = ((L.snake_dqn_plan, L.snake_dqn_rows) if plan == 'window' else
                        (L.snake_dqn_map_plan, L.snake_dqn_map_rows))
    check(plan_fn(ctypes.byref(cfg), ctypes.byref(lay)), L)
    H, W, C, A = int(h), int(w), int(c), int(A)
    P, P16, CP, K1 = H * W, lay.p16, lay.cpad, lay.k1
    d = torch.device(device)
    f32 = dict(dtype=torch.float32, device=d)

    def g(name):
        return state[name].detach().to(**f32)

    def bits(t):          # bf16 bit patterns as int16 (the kernels' uint16 words)
        return t.to(torch.bfloat16).contiguous().view(torch.int16)

    def conv_pack(w, cin_pad, k_pad):
        # [out][in][ky][kx] -> B[out][k = (ky*3 + kx) * cin_pad + ci], zero padded,
        # stored in MFMA fragment order: [out/16][k/32][k%32 / 8][out%16][8]
        out_ch, cin = w.shape[0], w.shape[1]
        t = torch.zeros((out_ch, 9, cin_pad), **f32)
        t[:, :, :cin] = w.permute(0, 2, 3, 1).reshape(out_ch, 9, cin)
        flat = torch.zeros((out_ch, k_pad), **f32)
        flat[:, :9 * cin_pad] = t.reshape(out_ch, 9 * cin_pad)
        frag = flat.reshape(out_ch // 16, 16, k_pad // 32, 4, 8).permute(0, 2, 3, 1, 4)
        return bits(frag.contiguous().reshape(out_ch, k_pad))

    w1, w2, w3 = g('conv1.weight'), g('conv2.weight'), g('conv3.weight')
    assert tuple(w1.shape) == (32, C, 3, 3) and tuple(w2.shape) == (64, 32, 3, 3) and tuple(w3.shape) == (64, 64, 3, 3)
    fc1 = g('fc1.weight')
    assert tuple(fc1.shape) == (256, 64 * P)
    # k in conv3's fragment order (snake_env.h snake_dqn_layout.fc1_w) -> the
    # reference's NCHW flatten index channel * h*w + position
    rows = (ctypes.c_int32 * P16)()
    n = rows_fn(ctypes.byref(cfg), ctypes.cast(rows, ctypes.c_void_p), P16)
    assert n == P16, n
    rowpos = torch.tensor(list(rows), dtype=torch.int64, device=d)
    k = torch.arange(64 * P16, device=d)
    r, j, c16, quad = k % 4, (k // 4) % 2, (k // 8) % 16, (k // 128) % 4
    half, m = (k // 512) % 2, k // 1024
    ch, p = (2 * half + j) * 16 + c16, rowpos[m * 16 + 4 * quad + r]
    src = torch.where(p >= 0, ch * P + p, 0)
    fc1p = torch.where((p >= 0)[None, :], fc1[:, src], torch.zeros((), **f32))
    fc3 = g('fc3.weight')
    assert tuple(fc3.shape) == (A, 128)
    tensors = dict(
        conv1_w=conv_pack(w1, CP, K1), conv2_w=conv_pack(w2, 32, 288), conv3_w=conv_pack(w3, 64, 576),
        fc1_w=bits(fc1p), fc2_w=bits(g('fc2.weight')),
        conv1_b=g('conv1.bias'), conv2_b=g('conv2.bias'), conv3_b=g('conv3.bias'),
        fc1_b=g('fc1.bias'), fc2_b=g('fc2.bias'), fc3_w=fc3.contiguous(), fc3_b=g('fc3.bias'))
    for k, n in (('conv1_w', lay.conv1_w), ('conv2_w', lay.conv2_w), ('conv3_w', lay.conv3_w),
                 ('fc1_w', lay.fc1_w), ('fc2_w', lay.fc2_w)):
        assert tensors[k].numel() == n, (k, tensors[k].numel(), n)
    return tensors
