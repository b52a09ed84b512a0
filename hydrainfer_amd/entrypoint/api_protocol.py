"""Request / chunk shapes of the chat-completions endpoint — the wire contract of
hydrainfer/entrypoint/api_protocol.py:6-52 (pydantic models there; plain dicts here) as
hydrainfer/entrypoint/api_server.py:89-152 uses them, and of the reference's own client
(benchmark/backend.py:13-64: it POSTs {model, messages: [{role, content: [text, image_url...]}], max_tokens,
temperature, stream: true} and reads `data: {json}` lines, `choices[0].delta.content`, until `data: [DONE]`).

Pinned to the reference by tests/golden/g13_api_protocol.json: the chunk strings the reference's pydantic models
produce (`model_dump_json(exclude_unset=True)`) and the prompt its LLaVA chat template renders, generated in the build
container by tests/golden/generate_goldens.py."""
import base64
import json
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional

from hydrainfer_amd.utils import keyword_argument

IMAGE_TOKEN = "<image>"            # hydrainfer/model/llava.py:195
CHUNK_OBJECT = "chat.completion.chunk"
MAX_TOP_LOGPROBS = 20              # OpenAI's limit
PROCESSED_LOGPROBS = "processed_logprobs"
LOGPROBS_MODES = ("raw_logprobs", PROCESSED_LOGPROBS)      # `logprobs_mode` (vLLM's names; engine/rcb.py)
MAX_STOP_TOKEN_IDS = 16
MAX_GUIDED_CHOICES = 64            # `guided_choice` (hydrainfer_amd/sampling)


class ProtocolError(ValueError):
    """A request the reference would reject (its asserts / pydantic validation -> HTTP 4xx / 500 there; 400 here)."""


@keyword_argument("guided_choice")
@keyword_argument("allowed_token_ids")
@keyword_argument("logprobs_mode")
@dataclass
class ChatRequest:
    model: str
    role: str
    text: str                       # message content with the image placeholders in front (api_server.py:62-79)
    image_png: Optional[bytes]      # decoded bytes of the (at most one) base64 PNG
    max_tokens: int
    stream: bool
    logprobs: bool = False          # OpenAI's `logprobs`: every chunk carries choices[0].logprobs
    top_logprobs: int = 0           # OpenAI's `top_logprobs`, 0..20; needs logprobs
    frequency_penalty: float = 0.0  # OpenAI's `frequency_penalty`, -2..2
    presence_penalty: float = 0.0   # OpenAI's `presence_penalty`, -2..2
    repetition_penalty: float = 1.0 # extension (the reference's process_logits step 2): > 0, 1 = none
    temperature: float = 0.0        # OpenAI's `temperature`, 0..2; absent means 0 (greedy) here, OpenAI's default is 1
    top_p: float = 1.0              # OpenAI's `top_p`, (0, 1]
    top_k: int = 0                  # extension (the reference's process_logits step 4): integer >= 0, 0 = off
    seed: Optional[int] = None      # OpenAI's `seed`, 0..2^63-1; absent: the engine assigns one
    # token constraints — keyword-only, declared ahead of prompt_logprobs (which stays the last field).  logit_bias:
    # OpenAI's, {"<token id>": bias in -100..100}, at most 300 entries; the other three are extensions under vLLM's names:
    # min_tokens (no end-of-sequence / stop token before this many tokens), min_p (0..1, sampled tokens have
    # p >= min_p * p_max; 0 = off), stop_token_ids (at most 16 ids that end the generation)
    logit_bias: Optional[Dict[int, float]] = field(default=None, kw_only=True)
    min_tokens: int = field(default=0, kw_only=True)
    min_p: float = field(default=0.0, kw_only=True)
    stop_token_ids: Optional[List[int]] = field(default=None, kw_only=True)
    # extension (vLLM's name): which distribution `logprobs` scores — absent / "raw_logprobs": the model's raw softmax (not
    # combinable with temperature > 0, penalties or constraints); "processed_logprobs": the one the token was chosen from
    # (init=False and the class's keyword_argument decorator: taken by keyword only, the generated signature as it was)
    logprobs_mode: Optional[str] = field(default=None, init=False)
    # extensions (vLLM's names), by keyword only like logprobs_mode; at most one of the two.  allowed_token_ids: the only
    # token ids the answer may consist of; guided_choice: strings of which the answer is exactly one (the server encodes
    # them with its tokenizer).  Not combinable with raw-mode logprobs; guided_choice not with min_tokens
    allowed_token_ids: Optional[List[int]] = field(default=None, init=False)
    guided_choice: Optional[List[str]] = field(default=None, init=False)
    prompt_logprobs: Optional[int] = None   # extension (vLLM's name; OpenAI's chat API has no `echo`): 0..20 — the stream's
                                            # first chunk carries the score of every prompt token, with that many alternatives


def parse_chat_completion_request(body: dict) -> ChatRequest:
    """ChatCompletionRequest (api_protocol.py:22-27) + the checks of create_chat_completion (api_server.py:95-99) +
    _parse_content (:62-79): every image_url content becomes one `<image>` placeholder IN FRONT of the text, followed by
    a newline; only `data:image/png;base64,` URLs; one message, at most one image."""
    if not isinstance(body, dict):
        raise ProtocolError("the request body must be a JSON object")
    model, messages = body.get("model"), body.get("messages")
    if not isinstance(model, str):
        raise ProtocolError("model: string required")
    if not isinstance(messages, list) or len(messages) != 1:
        raise ProtocolError("only support one round chat")                       # api_server.py:95
    msg = messages[0]
    role = msg.get("role") if isinstance(msg, dict) else None
    if role not in ("user", "system", "assistant"):
        raise ProtocolError("messages[0].role must be user / system / assistant")
    content = msg.get("content")
    text, images = "", []
    if isinstance(content, str):
        text_content, image_content = content, ""
    elif isinstance(content, list):
        text_content = image_content = ""
        for c in content:
            kind = c.get("type") if isinstance(c, dict) else None
            if kind == "text":
                text_content += c.get("text") or ""
            elif kind == "image_url":
                url = (c.get("image_url") or {}).get("url", "")
                prefix, _, b64 = url.partition(",")
                if prefix != "data:image/png;base64":
                    raise ProtocolError(f"only support base 64 png image url but got {prefix}")   # api_server.py:76
                image_content += IMAGE_TOKEN
                images.append(b64)
            else:
                raise ProtocolError("content type must be 'text' or 'image_url'")
    else:
        raise ProtocolError("messages[0].content: string or list required")
    if len(images) > 1:
        raise ProtocolError(f"only support one image per request, but got {len(images)} images")   # api_server.py:98
    text = image_content + "\n" + text_content if isinstance(content, list) else text_content
    max_tokens = body.get("max_tokens", 16)
    if max_tokens is None:
        max_tokens = 16
    if not isinstance(max_tokens, int) or isinstance(max_tokens, bool) or max_tokens < 1:
        raise ProtocolError("max_tokens: positive integer required")
    logprobs, top_logprobs = body.get("logprobs"), body.get("top_logprobs")
    if logprobs is None:
        logprobs = False
    if not isinstance(logprobs, bool):
        raise ProtocolError("logprobs: boolean required")
    if top_logprobs is None:
        top_logprobs = 0
    if not isinstance(top_logprobs, int) or isinstance(top_logprobs, bool) or not 0 <= top_logprobs <= MAX_TOP_LOGPROBS:
        raise ProtocolError(f"top_logprobs: integer 0..{MAX_TOP_LOGPROBS} required")
    if top_logprobs > 0 and not logprobs:
        raise ProtocolError("top_logprobs requires logprobs: true")
    logprobs_mode = body.get("logprobs_mode")
    if logprobs_mode is not None and logprobs_mode not in LOGPROBS_MODES:
        raise ProtocolError(f"logprobs_mode: one of {' / '.join(LOGPROBS_MODES)} required")
    if logprobs_mode == PROCESSED_LOGPROBS and not logprobs:
        raise ProtocolError(f"logprobs_mode: {PROCESSED_LOGPROBS} requires logprobs: true")
    raw_scores = logprobs and logprobs_mode != PROCESSED_LOGPROBS        # (the processed mode scores the choice itself)
    hint = f' (logprobs_mode: "{PROCESSED_LOGPROBS}" scores the token under the distribution it was chosen from)'
    penalties = {}
    for name in ("frequency_penalty", "presence_penalty"):
        v = body.get(name)
        if v is None:
            v = 0.0
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not -2.0 <= v <= 2.0:      # (a NaN fails the range)
            raise ProtocolError(f"{name}: number in -2..2 required")
        penalties[name] = float(v)
    v = body.get("repetition_penalty")
    if v is None:
        v = 1.0
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
        raise ProtocolError("repetition_penalty: number > 0 required")
    penalties["repetition_penalty"] = float(v)
    if raw_scores and (penalties["frequency_penalty"] or penalties["presence_penalty"] or v != 1):
        raise ProtocolError("logprobs cannot be combined with frequency / presence / repetition penalties yet" + hint)
    sampling = {}
    v = body.get("temperature")
    if v is None:
        v = 0.0
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= v <= 2.0:           # (a NaN fails the range)
        raise ProtocolError("temperature: number in 0..2 required")
    sampling["temperature"] = float(v)
    v = body.get("top_p")
    if v is None:
        v = 1.0
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 < v <= 1.0:
        raise ProtocolError("top_p: number in (0, 1] required")
    sampling["top_p"] = float(v)
    v = body.get("top_k")
    if v is None:
        v = 0
    if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= 0x7fffffff:
        raise ProtocolError("top_k: integer >= 0 required")
    sampling["top_k"] = v
    v = body.get("seed")
    if v is not None and (isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= (1 << 63) - 1):
        raise ProtocolError("seed: integer in 0..2^63-1 required")
    sampling["seed"] = v
    if raw_scores and sampling["temperature"] > 0:
        raise ProtocolError("logprobs cannot be combined with temperature > 0 yet" + hint)
    prompt_logprobs = body.get("prompt_logprobs")
    if prompt_logprobs is not None and (isinstance(prompt_logprobs, bool) or not isinstance(prompt_logprobs, int)
                                        or not 0 <= prompt_logprobs <= MAX_TOP_LOGPROBS):
        raise ProtocolError(f"prompt_logprobs: integer 0..{MAX_TOP_LOGPROBS} required")
    constraints = _parse_constraints(body)
    if raw_scores and (constraints["logit_bias"] or constraints["min_tokens"] > 0 or constraints["min_p"] > 0):
        raise ProtocolError("logprobs cannot be combined with logit_bias / min_tokens / min_p yet" + hint)
    masks = _parse_token_mask(body)
    if raw_scores and (masks["allowed_token_ids"] is not None or masks["guided_choice"] is not None):
        raise ProtocolError("logprobs cannot be combined with allowed_token_ids / guided_choice yet" + hint)
    if masks["guided_choice"] is not None and constraints["min_tokens"] > 0:
        raise ProtocolError("min_tokens cannot be combined with guided_choice: the answer ends where the choice ends")
    try:
        png = base64.b64decode(images[0], validate=True) if images else None
    except Exception:
        raise ProtocolError("image_url: invalid base64")
    return ChatRequest(model=model, role=role, text=text, image_png=png, max_tokens=max_tokens,
                       stream=bool(body.get("stream", False)), logprobs=logprobs, top_logprobs=top_logprobs, **penalties, **sampling,
                       prompt_logprobs=prompt_logprobs, logprobs_mode=logprobs_mode, **constraints, **masks)


def _parse_token_mask(body: dict) -> dict:
    """allowed_token_ids and guided_choice of a request body, as ChatRequest's fields (None where absent)."""
    allowed, choices = body.get("allowed_token_ids"), body.get("guided_choice")
    if allowed is not None and choices is not None:
        raise ProtocolError("allowed_token_ids and guided_choice cannot be combined")
    if allowed is not None:
        if not isinstance(allowed, list) or not allowed:
            raise ProtocolError("allowed_token_ids: non-empty list of token ids required")
        for t in allowed:
            if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t <= 0x7fffffff:
                raise ProtocolError("allowed_token_ids: integers >= 0 required")
        if len(set(allowed)) != len(allowed):
            raise ProtocolError("allowed_token_ids: a token id stands twice")
        allowed = list(allowed)
    if choices is not None:
        if not isinstance(choices, list) or not 1 <= len(choices) <= MAX_GUIDED_CHOICES:
            raise ProtocolError(f"guided_choice: list of 1..{MAX_GUIDED_CHOICES} strings required")
        for c in choices:
            if not isinstance(c, str) or not c:
                raise ProtocolError("guided_choice: non-empty strings required")
        if len(set(choices)) != len(choices):
            raise ProtocolError("guided_choice: a choice stands twice")
        choices = list(choices)
    return {"allowed_token_ids": allowed, "guided_choice": choices}


def _parse_constraints(body: dict) -> dict:
    """logit_bias, min_tokens, min_p and stop_token_ids of a request body, as ChatRequest's fields."""
    from hydrainfer_amd.sampling import MAX_LOGIT_BIAS
    logit_bias = body.get("logit_bias")
    if logit_bias is not None:
        if not isinstance(logit_bias, dict):
            raise ProtocolError("logit_bias: object of token id -> bias required")
        if len(logit_bias) > MAX_LOGIT_BIAS:
            raise ProtocolError(f"logit_bias: at most {MAX_LOGIT_BIAS} entries")
        table = {}
        for key, b in logit_bias.items():
            # (JSON keys are strings; OpenAI writes the token id in decimal.  isdecimal + isascii: no sign, no blank)
            if not isinstance(key, str) or not (key.isascii() and key.isdecimal()) or int(key) > 0x7fffffff:
                raise ProtocolError(f"logit_bias: key {key!r} is no token id (a non-negative integer as a decimal string)")
            if isinstance(b, bool) or not isinstance(b, (int, float)) or not -100.0 <= b <= 100.0:      # (a NaN fails the range)
                raise ProtocolError(f"logit_bias[{key!r}]: number in -100..100 required")
            table[int(key)] = float(b)
        if len(table) != len(logit_bias):
            raise ProtocolError("logit_bias: two keys name the same token id")
        logit_bias = table or None
    min_tokens = body.get("min_tokens")
    if min_tokens is None:
        min_tokens = 0
    if isinstance(min_tokens, bool) or not isinstance(min_tokens, int) or min_tokens < 0:
        raise ProtocolError("min_tokens: integer >= 0 required")
    min_p = body.get("min_p")
    if min_p is None:
        min_p = 0.0
    if isinstance(min_p, bool) or not isinstance(min_p, (int, float)) or not 0.0 <= min_p <= 1.0:       # (a NaN fails the range)
        raise ProtocolError("min_p: number in 0..1 required")
    stop = body.get("stop_token_ids")
    if stop is not None:
        if not isinstance(stop, list) or len(stop) > MAX_STOP_TOKEN_IDS:
            raise ProtocolError(f"stop_token_ids: list of at most {MAX_STOP_TOKEN_IDS} token ids required")
        for t in stop:
            if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t <= 0x7fffffff:
                raise ProtocolError("stop_token_ids: integers >= 0 required")
        stop = list(stop) or None
    return {"logit_bias": logit_bias, "min_tokens": min_tokens, "min_p": float(min_p), "stop_token_ids": stop}


def render_llava_chat_prompt(role: str, content: str, bos_token: str = "<s>", eos_token: str = "</s>") -> str:
    """hydrainfer/model/chat_template/template_llava.jinja with add_generation_prompt, for the one-message
    conversations the endpoint accepts (api_server.py:95): bos + [system text] + 'USER: ' + content + newline +
    'ASSISTANT:' + newline (the template's own line break after the generation prompt)."""
    if role == "system":
        return bos_token + content + "ASSISTANT:\n"
    if role != "user":
        raise ProtocolError("Conversation roles must alternate user/assistant/user/assistant/...")
    return bos_token + "USER: " + content + "\n" + "ASSISTANT:\n"


def _dumps(obj) -> str:
    return json.dumps(obj, separators=(",", ":"), ensure_ascii=False)      # pydantic's model_dump_json: compact, UTF-8


def _finite_or_none(x: float):
    """JSON has no literal for -inf / NaN (json.dumps would write the non-standard `-Infinity` / `NaN`): a logprob that
    is not a finite number — a masked (-inf) logit, a row that held a NaN — is sent as null."""
    return float(x) if math.isfinite(x) else None


def _token_logprob(token: str, logprob: float) -> dict:
    return {"token": token, "logprob": _finite_or_none(logprob), "bytes": list(token.encode("utf-8"))}


def chat_logprobs(token: str, logprob: float, alternatives) -> dict:
    """OpenAI's choices[0].logprobs for one generated token: {"content": [{token, logprob, bytes, top_logprobs:
    [{token, logprob, bytes}, ...]}]}; alternatives: the (token text, logprob) pairs, most likely first."""
    entry = _token_logprob(token, logprob)
    entry["top_logprobs"] = [_token_logprob(t, lp) for t, lp in alternatives]
    return {"content": [entry]}


def chat_prompt_logprobs(entries) -> list:
    """The `prompt_logprobs` array of a stream's first chunk, one element per token of the prompt: null (the first token:
    no context; an image placeholder), or {token, logprob, rank, bytes, top_logprobs: [{token, logprob, bytes}, ...]}.
    entries: None or (token text, logprob, rank, [(token text, logprob), ...]) per token; -inf / NaN -> null as in
    chat_logprobs."""
    out = []
    for e in entries:
        if e is None:
            out.append(None)
            continue
        token, logprob, rank, alternatives = e
        out.append({"token": token, "logprob": _finite_or_none(logprob), "rank": int(rank),
                    "bytes": list(token.encode("utf-8")),
                    "top_logprobs": [_token_logprob(t, lp) for t, lp in alternatives]})
    return out


def chat_stream_chunk(request_id: str, created: int, model: str, content: Optional[str], first: bool = False,
                      logprobs: Optional[dict] = None, prompt_logprobs: Optional[list] = None) -> str:
    """One `data:` line of the stream (api_server.py:119-146): the first chunk of a choice carries
    delta = {role: assistant, content: ""}, every other one delta = {content: text}; key order and `exclude_unset`
    as pydantic emits them.  logprobs: the chat_logprobs object of a request that asked for them (an extension: the
    reference has no such field); without it the chunk is byte for byte what it always was.  prompt_logprobs: the
    chat_prompt_logprobs array of a request that asked for it, on its first chunk (top level); the same holds."""
    delta = {"role": "assistant", "content": ""} if first else {"content": content}
    choice = {"index": 0, "delta": delta}
    if logprobs is not None:
        choice["logprobs"] = logprobs
    chunk = {"id": request_id, "object": CHUNK_OBJECT, "created": created, "model": model, "choices": [choice]}
    if prompt_logprobs is not None:         # top level, vLLM's place for it; only the first chunk of a request that asked
        chunk["prompt_logprobs"] = prompt_logprobs
    return "data: " + _dumps(chunk) + "\n\n"


DONE = "data: [DONE]\n\n"
