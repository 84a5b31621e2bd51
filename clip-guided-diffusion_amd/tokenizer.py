"""CLIP's byte-level BPE tokenizer (`clip.simple_tokenizer.SimpleTokenizer` and `clip.tokenize`), restated from the documented algorithm so
that prompts can be encoded without the `clip` package.

The algorithm (Radford et al. 2021, section 2.5; the GPT-2 byte-level BPE it builds on):
  - every byte maps to a printable unicode character (`bytes_to_unicode`), so BPE runs on strings without control or space characters;
  - the vocabulary is the 256 byte characters, the same 256 with the end-of-word marker `</w>`, one entry per merge of the merges file
    (lines 1 .. 49152 - 256 - 2 of `bpe_simple_vocab_16e6.txt.gz`; line 0 is a header), then `<|startoftext|>` and `<|endoftext|>`;
  - text is cleaned (HTML entities unescaped twice, whitespace collapsed, lower-cased), split by CLIP's pre-tokenisation pattern, and each
    piece is merged greedily by merge rank.
The one deviation: CLIP first runs `ftfy.fix_text` over the text.  `ftfy` is not a dependency here, so mojibake is not repaired; for
well-formed text (every ASCII prompt) the ids are the same.

`tokenize(texts, context_length=77, truncate=False)` returns an int64 (N, context_length) tensor: start token, the text's ids, end token, zero
padding; too long a text raises RuntimeError like `clip.tokenize`, or with truncate=True keeps the first context_length ids with the end token
in the last position.
"""
import functools
import gzip
import html
import os

import regex

BPE_FILENAME = "bpe_simple_vocab_16e6.txt.gz"
SOT, EOT = "<|startoftext|>", "<|endoftext|>"
_PATTERN = regex.compile(r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+""", regex.IGNORECASE)


def bpe_path(checkpoints_dir):
    """The merges file: $CGD_CLIP_BPE, else <checkpoints_dir>/clip/bpe_simple_vocab_16e6.txt.gz.  Nothing is downloaded."""
    env = os.environ.get("CGD_CLIP_BPE")
    default = os.path.join(checkpoints_dir, "clip", BPE_FILENAME)
    path = env or default
    if not os.path.isfile(path):
        raise FileNotFoundError(f"CLIP BPE merges file not found: looked at CGD_CLIP_BPE={env!r} and at {default} "
                                f"(copy {BPE_FILENAME} from the CLIP release to either place)")
    return path


@functools.lru_cache(maxsize=1)
def bytes_to_unicode():
    """byte -> printable character: the printable Latin-1 bytes map to themselves, the other 68 bytes to 256, 257, ... in byte order."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    table = {b: chr(b) for b in keep}
    extra = 0
    for b in range(256):
        if b not in table:
            table[b] = chr(256 + extra)
            extra += 1
    return table


def _clean(text):
    text = html.unescape(html.unescape(text)).strip()
    return regex.sub(r"\s+", " ", text).strip().lower()


class SimpleTokenizer:
    def __init__(self, path):
        with gzip.open(path, "rt", encoding="utf-8") as f:
            lines = f.read().split("\n")[1:49152 - 256 - 2 + 1]
        merges = [tuple(line.split()) for line in lines if line]
        byte_chars = list(bytes_to_unicode().values())
        vocab = byte_chars + [c + "</w>" for c in byte_chars] + ["".join(m) for m in merges] + [SOT, EOT]
        self.byte_encoder = bytes_to_unicode()
        self.encoder = {tok: i for i, tok in enumerate(vocab)}
        self.decoder = {i: tok for tok, i in self.encoder.items()}
        self.ranks = {m: i for i, m in enumerate(merges)}
        self.sot, self.eot = self.encoder[SOT], self.encoder[EOT]
        self._cache = {SOT: SOT, EOT: EOT}

    def bpe(self, token):
        """Space-separated BPE symbols of one pre-tokenised piece (already in byte characters)."""
        if token in self._cache:
            return self._cache[token]
        word = list(token[:-1]) + [token[-1] + "</w>"]
        while len(word) > 1:
            # the adjacent pair of lowest merge rank; merge every non-overlapping occurrence, left to right
            best, best_rank = None, None
            for pair in zip(word, word[1:]):
                r = self.ranks.get(pair)
                if r is not None and (best_rank is None or r < best_rank):
                    best, best_rank = pair, r
            if best is None:
                break
            merged, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == best[0] and word[i + 1] == best[1]:
                    merged.append(best[0] + best[1])
                    i += 2
                else:
                    merged.append(word[i])
                    i += 1
            word = merged
        out = " ".join(word)
        self._cache[token] = out
        return out

    def encode(self, text):
        ids = []
        for piece in _PATTERN.findall(_clean(text)):
            piece = "".join(self.byte_encoder[b] for b in piece.encode("utf-8"))
            ids.extend(self.encoder[s] for s in self.bpe(piece).split(" "))
        return ids

    def decode(self, ids):
        byte_decoder = {c: b for b, c in self.byte_encoder.items()}
        text = "".join(self.decoder[i] for i in ids)
        return bytearray(byte_decoder[c] for c in text).decode("utf-8", errors="replace").replace("</w>", " ")


@functools.lru_cache(maxsize=4)
def _tokenizer(path):
    return SimpleTokenizer(path)


def get_tokenizer(checkpoints_dir):
    return _tokenizer(bpe_path(checkpoints_dir))


def tokenize(texts, context_length=77, truncate=False, tokenizer=None, checkpoints_dir=None):
    """`clip.tokenize`: (N, context_length) int64, zero-padded.  `tokenizer` (a SimpleTokenizer) or `checkpoints_dir` (see bpe_path)."""
    import torch as th
    if tokenizer is None:
        if checkpoints_dir is None:
            raise ValueError("tokenize needs a tokenizer or the checkpoints directory that holds clip/" + BPE_FILENAME)
        tokenizer = get_tokenizer(checkpoints_dir)
    if isinstance(texts, str):
        texts = [texts]
    result = th.zeros(len(texts), context_length, dtype=th.int64)
    for i, text in enumerate(texts):
        ids = [tokenizer.sot] + tokenizer.encode(text) + [tokenizer.eot]
        if len(ids) > context_length:
            if not truncate:
                raise RuntimeError(f"Input {text} is too long for context length {context_length}")
            ids = ids[:context_length]
            ids[-1] = tokenizer.eot
        result[i, :len(ids)] = th.tensor(ids, dtype=th.int64)
    return result
