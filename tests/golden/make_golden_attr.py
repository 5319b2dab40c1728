#!/usr/bin/env python3
"""Golden vectors of the attribute-unlearning losses (utils.py:223-279: rbk, mmd_loss, buildLap).  Runs ONLY in the build
container, through make_golden's harness (the reference on sys.path): it drives the real reference in float32 with torch
autograd on rows of the toy user embedding kmeans_toy.npz['X'] (n = 1,508, d = 16) and writes data only, to attr_toy.npz
next to this script.

  cases [5, 3]                  (n1, n2, d) of each case: source X[:n1, :d], target X[n1:n1 + n2, :d]
  loss_{c}, grad_{c}            mmd_loss(source, target) (defaults: kernel_mul 2, kernel_num 5, no fix_sigma) and its autograd
                                gradient with respect to the n1 + n2 rows, float32
  u2u_shape (n1, n2, d), u2u_value
                                trace(U^T buildLap(n1 + n2, S, T) U), float32, U = X[:n1 + n2, :d]
  loop_{eta,alpha,lr,steps}, loop_rows
                                a d2d fine-tune on case 0 with the reference's mmd_loss and autograd in float32:
                                J = eta mmd_loss + alpha sum |U_i - U*_i|^2, `steps` plain gradient steps; the final rows

usage: python tests/golden/make_golden_attr.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (puts the reference on sys.path)

RU = MG.RU
torch = MG.torch
CASES = [(130, 170, 16), (1, 1, 16), (3, 70, 16), (65, 64, 5), (600, 908, 16)]
U2U = (5, 7, 16)
LOOP = dict(eta=1.0, alpha=0.05, lr=8.0, steps=3)


def gen_cases(X, out):
    out['cases'] = np.array(CASES, dtype=np.int64)
    for c, (n1, n2, d) in enumerate(CASES):
        rows = torch.tensor(X[:n1 + n2, :d].copy(), requires_grad=True)
        loss = RU.mmd_loss(rows[:n1], rows[n1:])
        grad, = torch.autograd.grad(loss, rows)
        out[f'loss_{c}'] = np.float32(loss.item())
        out[f'grad_{c}'] = grad.numpy().astype(np.float32)
        print(f'case {c} {(n1, n2, d)}: loss = {loss.item():.8g}, |grad|_max = {grad.abs().max().item():.4g}', flush=True)


def gen_u2u(X, out):
    n1, n2, d = U2U
    U = torch.tensor(X[:n1 + n2, :d].copy())
    lap = RU.buildLap(n1 + n2, list(range(n1)), list(range(n1, n1 + n2)))
    value = torch.trace(torch.mm(U.T, torch.mm(lap, U)))
    out['u2u_shape'] = np.array(U2U, dtype=np.int64)
    out['u2u_value'] = np.float32(value.item())
    print(f'u2u {U2U}: {value.item():.8g}', flush=True)


def gen_loop(X, out):
    n1, n2, d = CASES[0]
    T = torch.tensor(X[:n1 + n2, :d].copy(), requires_grad=True)
    start = T.detach().clone()
    for t in range(LOOP['steps']):
        J = LOOP['eta'] * RU.mmd_loss(T[:n1], T[n1:]) + LOOP['alpha'] * ((T - start) ** 2).sum()
        g, = torch.autograd.grad(J, T)
        with torch.no_grad():
            T -= LOOP['lr'] * g
        print(f'loop step {t}: J = {J.item():.8g}, moved {float((T.detach() - start).abs().max()):.4g}', flush=True)
    for k, v in LOOP.items():
        out[f'loop_{k}'] = np.array(v)
    out['loop_rows'] = T.detach().numpy().astype(np.float32)


if __name__ == '__main__':
    X = np.load(os.path.join(HERE, 'kmeans_toy.npz'))['X'].astype(np.float32)
    out = {}
    gen_cases(X, out)
    gen_u2u(X, out)
    gen_loop(X, out)
    np.savez_compressed(os.path.join(HERE, 'attr_toy.npz'), **out)
