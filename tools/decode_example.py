"""End-to-end decode on the MI355X path, the shape of the reference's recognize.py for this model family:
waveforms -> HIP fbank -> bidirectional RWKV encoder -> CTC (greedy / prefix beam search on the device) -> SentencePiece
tokens -> text -> WER report, with each token's frame where the search reports one (prefix beam search).  Random-init weights (no checkpoint can ship here), so the text is noise: the point is the
chain and its interfaces -- pass --checkpoint / --config of a real GigaSpeech model to decode for real.

  python tools/decode_example.py [--config conf.yaml --checkpoint model.pt --bpe_model spm.model --units units.txt]
                                 [--mode ctc_prefix_beam_search --context_list_path hotwords.txt --context_graph_score 3.0]
                                 [--stream 16]

--stream CHUNK decodes one utterance as a stream instead, from its AUDIO (utils.audio_stream.AudioStreamer): the default
model becomes the uni-directional encoder with a causal conv module, the waveform arrives in packets of 0.64 s, the streaming
fbank turns them into frames, the encoder runs window by window with carried state as soon as a window's frames exist, every
CHUNK output frames go through the streaming CTC search, and the committed text -- the tokens that can no longer change --
is printed as it grows, followed by the final result.
"""
import argparse, io, os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B                                                                  # noqa: E402
from paper_accurate_fast_cheap_amd.dataset.fbank import fbank_batch                 # noqa: E402
from paper_accurate_fast_cheap_amd.scoring.wer import WerScorer, giga_post_process  # noqa: E402
from paper_accurate_fast_cheap_amd.text import RevBpeTokenizer                      # noqa: E402
from paper_accurate_fast_cheap_amd.utils.init_model import init_model               # noqa: E402

G = os.path.join(ROOT, "tests", "golden", "text")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config"); ap.add_argument("--checkpoint")
    ap.add_argument("--bpe_model", default=os.path.join(G, "spm_tiny.model"))
    ap.add_argument("--units", default=os.path.join(G, "units.txt"))
    ap.add_argument("--mode", default="ctc_greedy_search", choices=["ctc_greedy_search", "ctc_prefix_beam_search"])
    ap.add_argument("--beam_size", type=int, default=8)
    ap.add_argument("--context_list_path", default="", help="hotword list, one phrase per line (prefix beam search)")
    ap.add_argument("--context_graph_score", type=float, default=0.0, help="bonus per matched hotword token")
    ap.add_argument("--stream", type=int, default=0, metavar="CHUNK", help="stream one utterance in chunks of CHUNK encoder frames")
    args = ap.parse_args(argv)
    dev = torch.device("cuda")
    tok = RevBpeTokenizer(args.bpe_model, args.units, None)
    if args.config:
        import yaml
        configs = yaml.safe_load(open(args.config))
    else:   # the paper's encoder shape with a vocabulary that matches the tiny tokenizer fixture
        conf = B.encoder_conf()
        if args.stream:      # a stream needs the uni-directional encoder; a causal conv module needs no look-ahead
            conf.update(selfattention_layer_type="rwkv_tmix60", rnn_att_direction="uni", causal=True, cnn_module_kernel=15)
        configs = dict(encoder="conformer", encoder_conf=conf, input_dim=80, output_dim=tok.vocab_size(),
                       ctc="ctc", ctc_conf={"ctc_blank_id": 0}, model_conf={}, dataset_conf={})

    class A:
        checkpoint = args.checkpoint

    torch.manual_seed(777)
    model, _ = init_model(A(), configs)
    model = model.eval().to(torch.bfloat16).to(dev)
    # three synthetic "utterances" (2.5 s, 4 s, 1.2 s) and made-up reference transcripts
    waves = [B.synthetic_waveform(s, 10 + i).to(dev) for i, s in enumerate((2.5, 4.0, 1.2))]
    refs = ["THE STATE-OF-THE-ART", "IT'S UH E-COMMERCE <COMMA> OKAY", "HELLO"]
    samples = [w.shape[1] for w in waves]
    padded = torch.zeros(len(waves), max(samples), device=dev)
    for i, w in enumerate(waves):
        padded[i, :samples[i]] = w[0]
    context_graph = None
    if args.context_list_path:
        from paper_accurate_fast_cheap_amd.utils.context_graph import ContextGraph
        context_graph = ContextGraph(args.context_list_path, tok.symbol_table, args.bpe_model, args.context_graph_score)
    if args.stream:
        return stream_one(model, tok, waves[1], args, context_graph)
    # one launch for the whole batch: (B, T_max, 80) bf16, zero behind every utterance's frames, and the frame counts
    batch, lens = fbank_batch(padded, samples, num_mel_bins=80, dither=0.0, out_dtype=torch.bfloat16)
    lens = lens.to(torch.int64)
    with torch.no_grad():
        results = model.decode([args.mode], batch, lens, beam_size=args.beam_size,
                               context_graph=context_graph)[args.mode]
    scorer = WerScorer()
    out = io.StringIO()
    for i, (r, ref) in enumerate(zip(results, refs)):
        text, pieces = tok.detokenize(list(r.tokens))
        al = scorer.add(f"utt{i}", giga_post_process(ref).split(), giga_post_process(text).split())
        out.write(f"utt{i}: {len(r.tokens)} tokens -> {text[:60]!r}   {al.counts.line()}\n")
        if r.times is not None:    # frame of each token (encoder frames after subsampling)
            out.write("  frames: " + " ".join(f"{t}:{f}" for t, f in zip(r.tokens, r.times)) + "\n")
    tot = scorer.overall()
    out.write("Overall -> %4.2f %% %s\n" % (tot.wer, tot.line()))
    print(out.getvalue(), end="")
    return results


PACKET = 10240     # 0.64 s of audio per feed


def stream_one(model, tok, wave, args, context_graph):
    from paper_accurate_fast_cheap_amd.utils.audio_stream import AudioStreamer
    shown = [0]

    def on_partial(i, partial, committed):
        if len(committed[0]) > shown[0]:
            shown[0] = len(committed[0])
            print(f"window {i:3d}: committed {shown[0]:3d} tokens -> {tok.detokenize(committed[0])[0][-60:]!r}"
                  f"   (1-best now {len(partial[0].tokens)} tokens)")

    streamer = AudioStreamer(model, 1, args.stream, args.mode, beam_size=args.beam_size, context_graph=context_graph,
                             on_partial=on_partial, max_total_frames=wave.shape[1] // 640 + args.stream)
    for a in range(0, wave.shape[1], PACKET):
        streamer.feed(wave[:, a:a + PACKET])
    results = streamer.finish()
    r = results[0]
    print(f"final: {len(r.tokens)} tokens -> {tok.detokenize(list(r.tokens))[0][:60]!r}")
    if r.times is not None:
        print("  frames: " + " ".join(f"{t}:{f}" for t, f in zip(r.tokens, r.times)))
    return results


if __name__ == "__main__":
    main()
