"""C5-shaped timing (BCH(1023,983,4), 0-4 distinct bit errors per codeword): encode and decode calls
(HIP events around each, the batch restored from a master copy before each decode), with a check
that the batch is restored.  The library is the default one or EZRS_LIB_VARIANT's.
--m M --t T --len L: the same for BCH(m, t) on rows of L data bytes with 0-T errors, packed with
the ECC inline; --separate-ecc: the ECC in an array of its own.
Usage: c5_decode_time.py [ncw] [reps] [--m M --t T --len L] [--separate-ecc]"""
import argparse, os, sys, time
import torch
sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "ezpwd-reed-solomon_amd"))
import ezrs

ap = argparse.ArgumentParser()
ap.add_argument("ncw", nargs="?", type=int, default=1 << 20)
ap.add_argument("reps", nargs="?", type=int, default=30)
ap.add_argument("--m", type=int)
ap.add_argument("--t", type=int)
ap.add_argument("--len", type=int)
ap.add_argument("--separate-ecc", action="store_true")
args = ap.parse_args()
ncw, reps = args.ncw, args.reps
if args.m is None:
    c, L = ezrs.BCH.nkt(1023, 983, 4), 122
else:
    c = ezrs.BCH(args.m, args.t)
    L = c.max_len if args.len is None else args.len
T, eb = c.t, c.ecc_bytes
row = L + eb
gen = torch.Generator(device="cuda").manual_seed(5)
clean = torch.randint(0, 256, (ncw, row), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8)
c.encode(clean, L)
nbits = 8 * L + c.ecc_bits
counts = torch.randint(0, T + 1, (ncw,), generator=gen, device="cuda", dtype=torch.int32)
pos = (torch.sort(torch.rand((ncw, T), generator=gen, device="cuda"), dim=1).values
       * (nbits - T + 1)).to(torch.int64) + torch.arange(T, device="cuda")
master = clean.clone()
flat = master.view(-1)
for j in range(T):
    r = torch.nonzero(counts > j).squeeze(1)
    p = pos[r, j]
    idx = r * row + p // 8
    flat[idx] = flat[idx] ^ (128 >> (p % 8)).to(torch.uint8)
res = torch.empty(ncw, dtype=torch.int32, device="cuda")
if args.separate_ecc:
    # contiguous data and ECC arrays; `work` keeps both for the final comparison
    cdata, cecc = clean[:, :L].contiguous(), clean[:, L:].contiguous()
    mdata, mecc = master[:, :L].contiguous(), master[:, L:].contiguous()
    wdata, wecc = torch.empty_like(mdata), torch.empty_like(mecc)

    def restore():
        wdata.copy_(mdata)
        wecc.copy_(mecc)

    def encode():
        c.encode(cdata, L, ecc=cecc)

    def decode():
        c.decode(wdata, L, ecc=wecc, result=res)
else:
    work = torch.empty_like(master)

    def restore():
        work.copy_(master)

    def encode():
        c.encode(clean, L)

    def decode():
        c.decode(work, L, result=res)
t0 = time.time()
while time.time() - t0 < 0.5:
    for _ in range(5):
        restore()
        decode()
    torch.cuda.synchronize()
ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
for e in ev:
    restore()
    e[0].record()
    encode()
    e[1].record()
    decode()
    e[2].record()
torch.cuda.synchronize()
enc = sum(e[0].elapsed_time(e[1]) for e in ev) / reps
dec = sum(e[1].elapsed_time(e[2]) for e in ev) / reps
if args.separate_ecc:
    work = torch.cat((wdata, wecc), dim=1)
ok = torch.equal(res, counts) and torch.equal(work, clean)
what = "" if args.m is None else f"codec={c!r} len={L} ecc={'separate' if args.separate_ecc else 'inline'} "
print(f"{what}ncw={ncw} encode_ms={enc:.4f} decode_ms={dec:.4f} ok={ok} "
      f"variant={os.path.basename(os.environ.get('EZRS_LIB_VARIANT', 'default'))}")
