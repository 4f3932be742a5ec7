"""OpenAI-style HTTP serving front-end for the local engine.

POST /v1/completions        prompt, max_tokens, temperature, top_k, top_p,
                            stop, n, stream (SSE), echo+logprobs (eval),
                            speculative, cache_prefix
POST /v1/chat/completions   messages=[{role, content}], ... (+ stream SSE)
POST /v1/sessions           open a paged continuous-batching session:
                            prompt, max_tokens, temperature, top_k, top_p,
                            seed (per session; defaults are greedy)
POST /v1/sessions/batch     open several sessions in shared ragged prefill
                            forwards (prompts=[...]); all or nothing. The
                            sampling fields are scalars for all prompts or
                            lists with one entry per prompt
POST /v1/sessions/step      advance all sessions (?n=K); reports the pool's
                            free_blocks and kv_dtype ("fp8" when the engine
                            was created with kv_quant="fp8")
GET  /v1/sessions/{id}      poll result (echoes the sampling parameters)
DELETE /v1/sessions/{id}    close
POST /v1/sessions/{id}/extend   continue a finished session (next turn);
                            a sampling field left out keeps the session's
GET  /v1/models             available ModelSpecs
GET  /health                engine + device status

One engine instance serves requests serially under a lock (the decode hot
path owns the GPU; concurrent multi-session serving is the
PagedSessionManager API, engine/sessions.py — an HTTP multiplexer over it
is a natural extension). The reference has no serving surface at all (its
"server" is the memdir HTTP API); this is engine-native.
"""

from __future__ import annotations

import threading
import time
from typing import List, Optional, Union

from pydantic import BaseModel

from fei_amd.engine.config import MODEL_SPECS
from fei_amd.engine.engine import LocalEngine


class CompletionRequest(BaseModel):
    prompt: str
    model: Optional[str] = None          # informational; engine is fixed
    max_tokens: int = 256
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    stop: Optional[List[str]] = None
    n: int = 1
    stop_on_eos: bool = True
    speculative: Optional[bool] = None
    stream: bool = False
    echo: bool = False
    logprobs: Optional[int] = None
    cache_prefix: bool = True


class ChatMessage(BaseModel):
    role: str
    content: str


class SessionOpen(BaseModel):
    prompt: str
    max_tokens: int = 256
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 0


class SessionOpenBatch(BaseModel):
    prompts: List[str]
    max_tokens: int = 256
    # one value for all prompts, or one per prompt
    temperature: Union[float, List[float]] = 0.0
    top_k: Union[int, List[int]] = 0
    top_p: Union[float, List[float]] = 1.0
    seed: Union[int, List[int]] = 0


class SessionExtend(BaseModel):
    prompt: str
    max_tokens: int = 256
    # None keeps the session's value
    temperature: Optional[float] = None
    top_k: Optional[int] = None
    top_p: Optional[float] = None
    seed: Optional[int] = None


class ChatRequest(BaseModel):
    messages: List[ChatMessage]
    model: Optional[str] = None
    max_tokens: int = 256
    temperature: float = 0.0
    top_k: int = 0
    top_p: float = 1.0
    stream: bool = False


def flatten_chat(messages: List[ChatMessage]) -> str:
    """Minimal chat template for the byte tokenizer (a real checkpoint
    would bring its own template)."""
    parts = [f"{m.role}: {m.content}" for m in messages]
    parts.append("assistant:")
    return "\n".join(parts)


def create_app(engine: Optional[LocalEngine] = None,
               model: str = "llama3-tiny",
               session_blocks: Optional[int] = None, **engine_kwargs):
    from fastapi import FastAPI

    app = FastAPI(title="fei_amd", version="0.1.0")
    eng = engine or LocalEngine.create(model, **engine_kwargs)
    lock = threading.Lock()
    model_name = eng.spec.name

    cache = {"ids": []}     # cross-request prefix cache (LCP, like the
                            # agent backend): repeated/extended prompts
                            # re-prefill only the delta

    def _generate(prompt: str, req) -> dict:
        # top_k / top_p requests take the same path as every other request
        # (the filter runs in the sampler kernel), so the prefix cache, stop
        # strings and stop_on_eos apply to them too
        with lock:
            ids = eng.tokenizer.encode(prompt)
            n = 0
            if getattr(req, "cache_prefix", True) and eng.B == 1:
                limit = min(len(cache["ids"]), len(ids) - 1)
                while n < limit and ids[n] == cache["ids"][n]:
                    n += 1
            try:
                out = eng.generate(
                    ids, max_new_tokens=req.max_tokens,
                    temperature=req.temperature,
                    stop_on_eos=getattr(req, "stop_on_eos", True),
                    speculative=getattr(req, "speculative", None),
                    stop=getattr(req, "stop", None),
                    from_pos=n, top_k=req.top_k, top_p=req.top_p)
            except ValueError as e:          # bad top_k / top_p
                from fastapi import HTTPException
                raise HTTPException(status_code=422, detail=str(e))
            # drop the final generated token: only sampled, its KV row
            # is never written (same rule as the agent backend)
            cache["ids"] = ids + list(out["token_ids"])[:-1]
        return out

    @app.get("/health")
    def health():
        return {"status": "ok", "model": model_name,
                "device": str(eng.device),
                "gpu": eng.is_gpu, "hip_graph": eng.use_graph}

    @app.get("/v1/models")
    def models():
        return {"object": "list",
                "data": [{"id": name, "object": "model",
                          "owned_by": "fei_amd",
                          "active": name == model_name}
                         for name in sorted(MODEL_SPECS)]}

    @app.post("/v1/completions")
    def completions(req: CompletionRequest):
        t0 = time.time()
        if req.echo and req.max_tokens == 0:
            # evaluation mode (lm-eval pattern): teacher-forced logprobs of
            # the prompt itself, no generation
            ids = eng.tokenizer.encode(req.prompt)
            with lock:
                # loglikelihood overwrites the KV caches from position 0:
                # the cross-request prefix cache no longer describes them
                cache["ids"] = []
                ll = eng.loglikelihood(ids[:1], ids[1:])
            return {
                "id": f"cmpl-{int(t0 * 1000)}",
                "object": "text_completion",
                "model": model_name,
                "choices": [{"index": 0, "text": req.prompt,
                             "finish_reason": "length",
                             "logprobs": {
                                 "token_logprobs": [None] + ll["token_logprobs"],
                                 "is_greedy": ll["is_greedy"],
                             }}],
                "usage": {"prompt_tokens": len(ids),
                          "completion_tokens": 0,
                          "total_tokens": len(ids)},
            }
        if req.stream:
            import json

            from fastapi.responses import StreamingResponse

            def sse():
                with lock:
                    # streaming prefills from position 0: invalidate the
                    # cross-request prefix cache
                    cache["ids"] = []
                    prev = ""
                    for c in eng.generate_stream(
                            req.prompt, max_new_tokens=req.max_tokens,
                            temperature=req.temperature,
                            stop_on_eos=req.stop_on_eos,
                            stop=req.stop, top_k=req.top_k,
                            top_p=req.top_p):
                        delta = c["text"][len(prev):]
                        prev = c["text"]
                        payload = {"object": "text_completion.chunk",
                                   "model": model_name,
                                   "choices": [{"index": 0, "text": delta,
                                                "finish_reason":
                                                "stop" if c["done"] else None}]}
                        yield f"data: {json.dumps(payload)}\n\n"
                yield "data: [DONE]\n\n"

            return StreamingResponse(sse(), media_type="text/event-stream")
        choices = []
        n_req = max(1, min(int(getattr(req, "n", 1)), 8))
        seed0 = eng.seed
        try:
            for i in range(n_req):
                if n_req > 1 and req.temperature > 0:
                    eng.seed = seed0 + i   # distinct samples per choice
                out = _generate(req.prompt, req)
                choices.append({"index": i, "text": out["text"],
                                "finish_reason": out.get("finish_reason",
                                                         "stop")})
        finally:
            eng.seed = seed0
        n_new = len(out["token_ids"])
        return {
            "id": f"cmpl-{int(t0 * 1000)}",
            "object": "text_completion",
            "created": int(t0),
            "model": model_name,
            "choices": choices,
            "usage": {"prompt_tokens": out.get("prompt_tokens", 0),
                      "completion_tokens": n_new,
                      "total_tokens": out.get("prompt_tokens", 0) + n_new},
            "metrics": {k: v for k, v in eng.last_metrics.items()
                        if isinstance(v, (int, float))},
        }

    @app.post("/v1/chat/completions")
    def chat(req: ChatRequest):
        t0 = time.time()
        if req.stream:
            import json

            from fastapi.responses import StreamingResponse

            prompt = flatten_chat(req.messages)

            def sse():
                with lock:
                    cache["ids"] = []       # stream prefills from position 0
                    prev = ""
                    for c in eng.generate_stream(
                            prompt, max_new_tokens=req.max_tokens,
                            temperature=req.temperature, top_k=req.top_k,
                            top_p=req.top_p):
                        delta = c["text"][len(prev):]
                        prev = c["text"]
                        payload = {"object": "chat.completion.chunk",
                                   "model": model_name,
                                   "choices": [{"index": 0,
                                                "delta": {"content": delta},
                                                "finish_reason":
                                                "stop" if c["done"] else None}]}
                        yield f"data: {json.dumps(payload)}\n\n"
                yield "data: [DONE]\n\n"

            return StreamingResponse(sse(), media_type="text/event-stream")
        out = _generate(flatten_chat(req.messages), req)
        return {
            "id": f"chatcmpl-{int(t0 * 1000)}",
            "object": "chat.completion",
            "created": int(t0),
            "model": model_name,
            "choices": [{"index": 0,
                         "message": {"role": "assistant",
                                     "content": out["text"]},
                         "finish_reason": "stop"}],
            "usage": {"prompt_tokens": out.get("prompt_tokens", 0),
                      "completion_tokens": len(out["token_ids"]),
                      "total_tokens": (out.get("prompt_tokens", 0) +
                                       len(out["token_ids"]))},
        }

    # -- multi-session serving (paged continuous batching) -------------------

    state = {"mgr": None}

    def _mgr():
        if state["mgr"] is None:
            from fei_amd.engine.sessions import PagedSessionManager
            # the pool inherits the engine's kv_quant (an fp8 engine serves
            # its sessions out of fp8 blocks)
            state["mgr"] = PagedSessionManager(eng, num_blocks=session_blocks)
        return state["mgr"]

    @app.post("/v1/sessions")
    def session_open(req: SessionOpen):
        from fastapi import HTTPException
        with lock:
            try:
                sid = _mgr().open(req.prompt, max_new_tokens=req.max_tokens,
                                  temperature=req.temperature,
                                  top_k=req.top_k, top_p=req.top_p,
                                  seed=req.seed)
            except ValueError as e:          # bad sampling parameter
                raise HTTPException(status_code=400, detail=str(e))
            except MemoryError as e:
                raise HTTPException(status_code=503, detail=str(e))
        return {"session_id": sid}

    @app.post("/v1/sessions/batch")
    def session_open_batch(req: SessionOpenBatch):
        """Open several sessions in shared ragged prefill forwards
        (PagedSessionManager.open_many): 400 on an empty list, an empty
        prompt, a bad sampling parameter or a parameter list whose length is
        not len(prompts); 503 on pool exhaustion. NOTHING is admitted then."""
        from fastapi import HTTPException
        if not req.prompts:
            raise HTTPException(status_code=400, detail="prompts is empty")
        with lock:
            try:
                sids = _mgr().open_many(req.prompts,
                                        max_new_tokens=req.max_tokens,
                                        temperature=req.temperature,
                                        top_k=req.top_k, top_p=req.top_p,
                                        seed=req.seed)
            except ValueError as e:
                raise HTTPException(status_code=400, detail=str(e))
            except MemoryError as e:
                raise HTTPException(status_code=503, detail=str(e))
        return {"session_ids": sids}

    @app.post("/v1/sessions/step")
    def session_step(n: int = 1):
        with lock:
            mgr = _mgr()
            # chunked stepping: ONE host sync for the whole request
            # (engine/sessions.step_chunk) instead of one per step
            advanced = mgr.step_chunk(max(1, n))
        return {"active": advanced,
                "open": len(mgr.sessions),
                "free_blocks": mgr.pool.free_blocks(),
                "kv_dtype": mgr.pool.kv_dtype}

    @app.get("/v1/sessions/{sid}")
    def session_get(sid: int):
        from fastapi import HTTPException
        mgr = _mgr()
        if sid not in mgr.sessions:
            raise HTTPException(status_code=404, detail="no such session")
        return {"session_id": sid, **mgr.result(sid)}

    @app.post("/v1/sessions/{sid}/extend")
    def session_extend(sid: int, req: SessionExtend):
        """Continue a finished session with new prompt tokens (the next
        turn): 404 unknown session, 409 still decoding, 400 context
        overflow or a bad sampling parameter, 503 pool exhausted (the
        session is left untouched)."""
        from fastapi import HTTPException
        with lock:
            mgr = _mgr()
            if sid not in mgr.sessions:
                raise HTTPException(status_code=404, detail="no such session")
            if not mgr.sessions[sid].done:
                raise HTTPException(status_code=409,
                                    detail="session is still active")
            try:
                first = mgr.extend(sid, req.prompt,
                                   max_new_tokens=req.max_tokens,
                                   temperature=req.temperature,
                                   top_k=req.top_k, top_p=req.top_p,
                                   seed=req.seed)
            except ValueError as e:          # context overflow, bad parameter
                raise HTTPException(status_code=400, detail=str(e))
            except MemoryError as e:
                raise HTTPException(status_code=503, detail=str(e))
        return {"session_id": sid, "first_token": first}

    @app.delete("/v1/sessions/{sid}")
    def session_close(sid: int):
        with lock:
            _mgr().close(sid)
        return {"closed": sid}

    app.state.engine = eng
    app.state.session_manager = _mgr      # callable: built on first use
    return app


def main(argv=None) -> int:
    import argparse

    import uvicorn

    p = argparse.ArgumentParser("fei-api",
                                description="OpenAI-style local serving API")
    p.add_argument("--model", default=None,
                   help="default: llama3-8b on GPU, llama3-tiny on CPU")
    p.add_argument("--host", default="127.0.0.1")
    p.add_argument("--port", type=int, default=8123)
    p.add_argument("--check", action="store_true",
                   help="build the app (loads the model) and exit")
    args = p.parse_args(argv)
    if args.model is None:
        import torch
        args.model = ("llama3-8b" if torch.cuda.is_available()
                      else "llama3-tiny")
    app = create_app(model=args.model)
    if args.check:
        print(f"[fei-api] ok: {app.state.engine.spec.name} on "
              f"{app.state.engine.device}")
        return 0
    uvicorn.run(app, host=args.host, port=args.port)
    return 0


if __name__ == "__main__":
    main()
