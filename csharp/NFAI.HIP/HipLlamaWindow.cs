// Lossless greedy speculative decoding from a C# host: up to 8 CONSECUTIVE positions of ONE model per pass over the weights
// (nfai_hip_llama_window_*).  The reference emits one token per pass of the loop LlamaModel.cs:116-125; with SamplingUtils.ArgMax
// (SamplingUtils.cs:43-57) the next tokens are a function of the sequence alone, so guessed continuations ride as extra columns of
// the batched kernels and are kept exactly as far as the model's own ArgMax agrees.  NOT compiled in this repository.
namespace NFAI.HIP;

public sealed unsafe class HipLlamaWindow : IDisposable
{
    private ulong handle;
    public uint MaxTokens { get; }
    public uint Vocab { get; }

    /// <summary>model: a finalized, whole model of the fused path (HipLlamaModel.Handle); maxTokens in [2, 8].  quantized: its matrices
    /// are all Q4_K / Q6_K (Q4_K_M files, NFAI_BATCH_QUANT) instead of all fp16; anyQuant (with quantized): Q5_K,
    /// Q8_0, Q4_0, Q3_K and IQ4_XS matrices too (Q5_K_M, Q8_0, Q4_0, Q3_K_S/M and IQ4_XS files, NFAI_BATCH_QUANT_ANY).  The window owns the columns' activation vectors, its
    /// workspaces and graphs, no weights and no KV cache; the model stays a normal model between window calls.  Throws with tensor and
    /// type for Q5_K / Q8_0 / Q4_0 / Q3_K / IQ4_XS weights without anyQuant, pipeline stages, the 1:1 or engine path.</summary>
    public HipLlamaWindow(ulong model, uint maxTokens, uint vocab, bool quantized = false, bool anyQuant = false)
    {
        if (anyQuant && !quantized) throw new ArgumentException("anyQuant widens quantized and needs it", nameof(anyQuant));
        MaxTokens = maxTokens; Vocab = vocab;
        Native.Check(Native.nfai_hip_llama_window_create(model, maxTokens, (quantized ? BatchQuant : 0u) | (anyQuant ? BatchQuantAny : 0u), out handle));
    }

    private const uint BatchQuant = 1u;   // NFAI_BATCH_QUANT (nfai_hip.h)
    private const uint BatchQuantAny = 4u;   // NFAI_BATCH_QUANT_ANY

    /// <summary>tokens[i] at position p + i (tokens.Length passes of LlamaModel.cs:116-125 on the caller's tokens): argmax[i] is the first
    /// index of column i's largest logit (SamplingUtils.cs:55-56); logits is [tokens.Length][Vocab] or empty.  The position advances
    /// by tokens.Length.  One graph launch and one synchronisation.</summary>
    public void Step(ReadOnlySpan<uint> tokens, Span<float> logits, Span<uint> argmax)
    {
        if (tokens.Length < 1 || tokens.Length > MaxTokens) throw new ArgumentException("1 to MaxTokens tokens per step", nameof(tokens));
        if (!argmax.IsEmpty && argmax.Length != tokens.Length) throw new ArgumentException("one argmax slot per token, or empty", nameof(argmax));
        if (!logits.IsEmpty && logits.Length != tokens.Length * Vocab) throw new ArgumentException("logits is [tokens][Vocab] or empty", nameof(logits));
        fixed (uint* t = tokens) fixed (float* l = logits) fixed (uint* a = argmax)
            Native.Check(Native.nfai_hip_llama_window_step(handle, t, (uint)tokens.Length, logits.IsEmpty ? null : l, argmax.IsEmpty ? null : a));
    }

    /// <summary>`token` and the guessed tokens behind it in one pass; returns how many tokens were emitted into tokensOut
    /// (1 to draft.Length + 1): exactly what that many plain greedy steps from `token` would return (SamplingUtils.cs:43-57).
    /// Afterwards the model is where those steps would have left it.  A loop that ends at EOS never feeds it (LlamaModel.cs:116-125
    /// stops with the position in front of it), so EOS must not ride as a draft: PromptLookupDrafter.Propose(..., stop: eos).</summary>
    public uint Verify(uint token, ReadOnlySpan<uint> draft, Span<uint> tokensOut)
    {
        if (draft.Length + 1 > MaxTokens) throw new ArgumentException("at most MaxTokens - 1 drafts", nameof(draft));
        if (tokensOut.Length < draft.Length + 1) throw new ArgumentException("tokensOut holds draft.Length + 1 tokens", nameof(tokensOut));
        uint n;
        fixed (uint* d = draft) fixed (uint* o = tokensOut)
            Native.Check(Native.nfai_hip_llama_window_verify(handle, token, draft.IsEmpty ? null : d, (uint)draft.Length, null, o, &n));
        return n;
    }

    /// <summary>Algorithmic HBM bytes of one window step of t tokens at the model's position: every weight once, the cached K / V rows once.</summary>
    public ulong BytesPerStep(uint t)
    {
        ulong total;
        Native.Check(Native.nfai_hip_llama_window_bytes_per_step(handle, t, &total));
        return total;
    }

    /// <summary>One window step launch by launch between events: (milliseconds, launches) per kernel class
    /// (0 qkv, 1 attn, 2 wo, 3 gateup, 4 down, 5 lmhead, 6 other).  The position advances by tokens.Length.</summary>
    public (float[] Ms, uint[] Launches) ProfileStep(ReadOnlySpan<uint> tokens)
    {
        var ms = new float[8]; var n = new uint[8];
        fixed (uint* t = tokens) fixed (float* m = ms) fixed (uint* c = n)
            Native.Check(Native.nfai_hip_llama_window_profile_step(handle, t, (uint)tokens.Length, m, c));
        return (ms, n);
    }

    public void Dispose()
    {
        if (handle == 0) return;
        Native.Check(Native.nfai_hip_llama_window_destroy(handle));
        handle = 0;
    }
}

/// <summary>Draft tokens without a second model: the tokens that followed the most recent earlier occurrence of the last n tokens of
/// the conversation, for the largest n in ngramMax .. 1 that occurs at all (prompt lookup).  Pure host code: a wrong guess costs
/// time, never correctness.</summary>
public sealed class PromptLookupDrafter
{
    private readonly int ngramMax;
    public PromptLookupDrafter(int ngramMax = 3) { this.ngramMax = Math.Max(1, ngramMax); }

    /// <summary>At most k tokens, ending where the history ends and in front of the first `stop` token.</summary>
    public uint[] Propose(IReadOnlyList<uint> history, int k, uint? stop = null)
    {
        int L = history.Count;
        if (k <= 0 || L < 2) return Array.Empty<uint>();
        for (int n = Math.Min(ngramMax, L - 1); n >= 1; n--)
            for (int start = L - n - 1; start >= 0; start--)
            {
                bool same = true;
                for (int j = 0; same && j < n; j++) same = history[start + j] == history[L - n + j];
                if (!same) continue;
                int len = Math.Min(k, L - (start + n));
                for (int j = 0; stop.HasValue && j < len; j++)
                    if (history[start + n + j] == stop.Value) len = j;
                var outp = new uint[len];
                for (int j = 0; j < len; j++) outp[j] = history[start + n + j];
                return outp;
            }
        return Array.Empty<uint>();
    }
}
