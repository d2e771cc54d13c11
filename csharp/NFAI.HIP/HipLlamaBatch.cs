// Several sequences decoded in one step from a C# host: n models over ONE set of weights (a donor and models made with
// nfai_hip_llama_share_tensors) advance one token each while every weight row is streamed from HBM once (nfai_hip_llama_batch_*).
// The reference serves one sequence per LlamaModel (the token loop LlamaModel.cs:116-125); n conversations are n RunAsync loops of one
// provider, each streaming all the weights again.  NOT compiled in this repository.
namespace NFAI.HIP;

public sealed unsafe class HipLlamaBatch : IDisposable
{
    private ulong handle;
    public uint Count { get; }
    public uint Vocab { get; }

    /// <summary>models: 1 to 8 distinct, finalized, whole fp16 models of one HipBufferManager that read the same tensors
    /// (HipLlamaModel.Handle).  The batch owns a workspace and its graphs, no weights and no KV cache: creating one is cheap, and a
    /// host whose sequence has ended disposes the batch and makes a smaller one.  Throws with the member and the reason for
    /// K-quant weights (unless quantized), pipeline stages, mixed KV types, separate weights, duplicates.</summary>
    /// quantized: also admits members whose matrices are all Q4_K / Q6_K (Q4_K_M files) through nfai_hip_llama_batch_create_ex with
    /// NFAI_BATCH_QUANT: every quantised row is read and unpacked once per step and multiplied on the matrix cores for all members.
    /// anyQuant (with quantized): Q5_K, Q8_0, Q4_0, Q3_K and IQ4_XS matrices too (Q5_K_M, Q8_0, Q4_0, Q3_K_S/M and IQ4_XS files, NFAI_BATCH_QUANT_ANY), in any per-tensor mix.
    /// wide: 1 to 16 whole fp16 models on the fp16-MFMA kernels (nfai_hip_llama_batch_create_wide); every method takes spans of Count.
    public HipLlamaBatch(ReadOnlySpan<ulong> models, uint vocab, bool quantized = false, bool anyQuant = false, bool wide = false)
    {
        if (anyQuant && !quantized) throw new ArgumentException("anyQuant widens quantized and needs it", nameof(anyQuant));
        if (wide && quantized) throw new ArgumentException("a wide batch takes fp16 models only", nameof(wide));
        Count = (uint)models.Length; Vocab = vocab;
        fixed (ulong* p = models)
            Native.Check(wide ? Native.nfai_hip_llama_batch_create_wide(p, Count, 0u, out handle)
                       : quantized ? Native.nfai_hip_llama_batch_create_ex(p, Count, BatchQuant | (anyQuant ? BatchQuantAny : 0u), out handle)
                                   : Native.nfai_hip_llama_batch_create(p, Count, out handle));
    }

    private const uint BatchQuant = 1u;   // NFAI_BATCH_QUANT (nfai_hip.h)
    private const uint BatchQuantAny = 4u;   // NFAI_BATCH_QUANT_ANY

    /// <summary>One token per member (one pass of LlamaModel.cs:116-125 for every sequence): tokens[i] runs at member i's own position
    /// in member i's own cache; argmax[i] is the first index of member i's largest logit (SamplingUtils.cs:55-56).  logits: Count * Vocab
    /// floats for hosts that sample themselves, or empty.  One graph launch and one synchronisation for all members.</summary>
    public void Step(ReadOnlySpan<uint> tokens, Span<float> logits, Span<uint> argmax)
    {
        if (tokens.Length != Count || argmax.Length != Count) throw new ArgumentException("one token and one argmax slot per member");
        if (!logits.IsEmpty && logits.Length != Count * Vocab) throw new ArgumentException("logits is [Count][Vocab] or empty", nameof(logits));
        fixed (uint* t = tokens) fixed (float* l = logits) fixed (uint* a = argmax)
            Native.Check(Native.nfai_hip_llama_batch_step(handle, t, logits.IsEmpty ? null : l, a));
    }

    /// <summary>One token per member as Step (LlamaModel.cs:116-125), then every member's candidates of the reference's default sampler
    /// formed on the device (SamplingUtils.cs:5-13: values / temperature, softmax over Vocab, stable descending order, Take(k)):
    /// ids[i * k ..] and probs[i * k ..] are member i's k most probable tokens, what nfai_hip_llama_decode_topk returns for one model.
    /// One graph launch and one synchronisation; 520 bytes per member cross PCIe instead of Vocab floats.</summary>
    public void StepTopK(ReadOnlySpan<uint> tokens, float temperature, uint k, Span<uint> ids, Span<float> probs)
    {
        if (tokens.Length != Count) throw new ArgumentException("one token per member", nameof(tokens));
        if (ids.Length != Count * k || probs.Length != Count * k) throw new ArgumentException("ids and probs are [Count][k]");
        fixed (uint* t = tokens) fixed (uint* i = ids) fixed (float* p = probs)
            Native.Check(Native.nfai_hip_llama_batch_step_topk(handle, t, temperature, k, i, p));
    }

    private const uint TopK = 40;                                   // SamplingUtils.cs:5 defaults
    private const float Temperature = 0.5f, TopPValue = 0.95f;

    /// <summary>One token per member with the reference's default sampler (LlamaModel.cs:128-130,165): StepTopK, then per member, in
    /// member order, the nucleus cut and the draw of SamplingUtils.cs:14-31 with Random.Shared.NextSingle().  next[i] is member i's
    /// sampled token.</summary>
    public void StepSampled(ReadOnlySpan<uint> tokens, Span<uint> next)
    {
        if (next.Length != Count) throw new ArgumentException("one slot per member", nameof(next));
        var ids = new uint[Count * TopK]; var probs = new float[Count * TopK];
        StepTopK(tokens, Temperature, TopK, ids, probs);
        for (int i = 0; i < Count; i++)
            next[i] = HipLlamaModel.TopPFromCandidates(ids.AsSpan(i * (int)TopK, (int)TopK).ToArray(), probs.AsSpan(i * (int)TopK, (int)TopK).ToArray(),
                                                       TopPValue, Random.Shared.NextSingle());
    }

    /// <summary>nSteps tokens per member with every member's ArgMax fed back on the device (SamplingUtils.cs:43-57 in place of TopP):
    /// tokensOut[s * Count + i] is member i's token after step s.</summary>
    public void Greedy(ReadOnlySpan<uint> firstTokens, uint nSteps, Span<uint> tokensOut)
    {
        if (firstTokens.Length != Count || tokensOut.Length != nSteps * Count) throw new ArgumentException("tokensOut is [nSteps][Count]");
        fixed (uint* f = firstTokens) fixed (uint* o = tokensOut)
            Native.Check(Native.nfai_hip_llama_batch_greedy(handle, f, nSteps, o));
    }

    /// <summary>Algorithmic HBM bytes of one batch step at the members' current positions: every weight once + per member its KV rows.</summary>
    public ulong BytesPerToken()
    {
        ulong total;
        Native.Check(Native.nfai_hip_llama_batch_bytes_per_token(handle, &total));
        return total;
    }

    /// <summary>One batch step launch by launch between events: (milliseconds, launches) per kernel class
    /// (0 qkv, 1 attn, 2 wo, 3 gateup, 4 down, 5 lmhead, 6 other).  Every member advances by one token.</summary>
    public (float[] Ms, uint[] Launches) ProfileStep(ReadOnlySpan<uint> tokens)
    {
        if (tokens.Length != Count) throw new ArgumentException("one token per member", nameof(tokens));
        var ms = new float[8]; var n = new uint[8];
        fixed (uint* t = tokens) fixed (float* m = ms) fixed (uint* c = n)
            Native.Check(Native.nfai_hip_llama_batch_profile_step(handle, t, m, c));
        return (ms, n);
    }

    public void Dispose()
    {
        if (handle == 0) return;
        Native.Check(Native.nfai_hip_llama_batch_destroy(handle));
        handle = 0;
    }
}
