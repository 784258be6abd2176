"""Sample from a GPT-2 or Llama checkpoint written by `workloads.py` / `train_flow.py`.

    python -m ray_torch_distributed_checkpoint_amd.generate --model gpt2-tiny --checkpoint DIR \\
        [--prompt-ids 1,2,3 | --prompt-len 16] --max-new-tokens 32 [--temperature --top-k --seed --batch]
        [--few-row] [--captured] [--fast]

Builds the model, loads the "model" part of the DCP checkpoint directory (what
`workloads.restore(mode="weights")` loads) and runs `model.generate()` (KV cache, split-KV decode
kernel on the GPU).  There is no tokenizer in the tree: the prompt is a list of token ids, or
`--prompt-len` tokens of each of the first `--batch` rows of the workloads' SyntheticTokens.
`--few-row` runs the decode linears on the weight-streaming few-row kernel (batch <= 16),
`--captured` replays the decode step from a hipGraph (GPU only), `--fast` sets both.
Prints one JSON line: the token ids and the tokens per second.
"""
from __future__ import annotations

import argparse
import json
import time

import torch

from .checkpoint import dcp
from .checkpoint.state_dict import get_state_dict, set_state_dict


def build_model(name: str, device):
    if name.startswith("llama"):
        from .models import Llama, LlamaConfig

        return Llama(LlamaConfig.named(name), device=device)
    if name.startswith("gpt2"):
        from .models import GPT2, GPT2Config

        return GPT2(GPT2Config.named(name)).to(device)
    raise ValueError(f"generate: {name!r} is not a language model of this package (gpt2*, llama*)")


def load_weights(model, path: str) -> None:
    """The "model" entry of a DCP checkpoint directory into the live model."""
    msd, _ = get_state_dict(model, None)
    sd = dcp.load({"model": msd}, path)
    set_state_dict(model, None, model_state_dict=sd["model"])


def prompt_tokens(args, vocab: int, device) -> torch.Tensor:
    if args.prompt_ids:
        ids = [int(t) for t in args.prompt_ids.split(",") if t.strip() != ""]
        if not ids or min(ids) < 0 or max(ids) >= vocab:
            raise ValueError(f"generate: --prompt-ids must be token ids in [0, {vocab})")
        return torch.tensor([ids] * args.batch, dtype=torch.int64, device=device)
    from .workloads import SyntheticTokens

    data = SyntheticTokens(max(args.batch, 1), args.prompt_len, vocab, seed=args.seed)
    return data.batch(torch.arange(args.batch, device=device))[0]


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="generate tokens from a GPT-2 / Llama checkpoint with a KV cache")
    ap.add_argument("--model", default="gpt2-tiny")
    ap.add_argument("--checkpoint", default=None, help="DCP checkpoint directory (default: the random init)")
    ap.add_argument("--prompt-ids", default=None, help="comma-separated token ids (every batch row gets them)")
    ap.add_argument("--prompt-len", type=int, default=16, help="without --prompt-ids: synthetic tokens per row")
    ap.add_argument("--max-new-tokens", type=int, default=32)
    ap.add_argument("--temperature", type=float, default=0.0, help="0: greedy")
    ap.add_argument("--top-k", type=int, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--eos-id", type=int, default=None)
    ap.add_argument("--sliding-window", type=int, default=None)
    ap.add_argument("--device", default=None, help="default: cuda when available")
    ap.add_argument("--few-row", action="store_true", help="decode linears on the few-row kernel (batch <= 16)")
    ap.add_argument("--captured", action="store_true", help="replay the decode step from a hipGraph (GPU only)")
    ap.add_argument("--fast", action="store_true", help="--few-row and --captured")
    args = ap.parse_args(argv)
    if args.fast:
        args.few_row = args.captured = True
    return args


def main(argv=None):
    args = parse_args(argv)
    device = torch.device(args.device or ("cuda" if torch.cuda.is_available() else "cpu"))
    torch.manual_seed(args.seed)
    model = build_model(args.model, device)
    if args.checkpoint:
        load_weights(model, args.checkpoint)
    model.eval()
    model.sliding_window = int(args.sliding_window) if args.sliding_window else None
    idx = prompt_tokens(args, model.cfg.vocab_size, device)
    if device.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = model.generate(idx, args.max_new_tokens, temperature=args.temperature, top_k=args.top_k, seed=args.seed,
                         eos_id=args.eos_id, few_row=args.few_row, captured=args.captured)
    tokens = out.tolist()  # (the device is read here, once)
    dt = time.perf_counter() - t0
    row = {"model": args.model, "device": device.type, "batch": idx.shape[0], "prompt_len": idx.shape[1],
           "new_tokens": args.max_new_tokens, "few_row": args.few_row, "captured": args.captured, "tokens": tokens,
           "tokens_per_s": round(idx.shape[0] * args.max_new_tokens / dt, 2) if dt > 0 else None}
    print(json.dumps(row))
    return row


if __name__ == "__main__":
    main()
