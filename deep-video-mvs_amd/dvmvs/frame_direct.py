"""The destination-passing frame body (one sequence per engine, the headline configuration): every producer writes straight into the buffer its
consumer reads -- FPN outputs, the cost volume and encoder outputs into channel slices of the encoder's concatenation buffers, skip connections and
up-sampled maps into the decoder's, the warped hidden state into the ConvLSTM's input, the gates into the state buffers in place, the last
convolution's epilogue into the depth buffer that is also next frame's "previous depth".  ``DirectFrameBody`` owns those buffers (two sets: frames
alternate, so that the next frame's state-free stages can run a frame ahead on a side stream) and launches the frame on them; what it is captured
into, and when, is ``dvmvs.engine``'s business."""
import torch

from dvmvs.fused_layers import FusedConv2d
from dvmvs.hip import ops as _ops


class DirectFrameBody:
    """One frame of pairnet (``lstm_fusion`` None) or fusionnet on the network's (BN-folded, epilogue-fused) modules and the frame's parameter
    block ``block`` (dvmvs.parameter_block.ParameterBlock: sizes, depth range, pose-algebra mode, the device views of the frame's matrices)."""

    def __init__(self, feature_extractor, feature_shrinker, cost_volume_encoder, lstm_fusion, cost_volume_decoder, block, device,
                 bottleneck_convs, sweep_mfma):
        self.fe, self.fs, self.enc, self.lstm, self.dec = feature_extractor, feature_shrinker, cost_volume_encoder, lstm_fusion, cost_volume_decoder
        self.block, self.device = block, device
        self.bottleneck_convs, self.sweep_mfma = bottleneck_convs, sweep_mfma
        self.is_fusionnet = lstm_fusion is not None
        self.buffers = {}      # see allocate; "sets": the two buffer sets
        self.h, self.c, self.prev_depth = None, None, None      # the recurrent state and the depth / previous-depth buffer
        self.side_stream = torch.cuda.Stream(device=device)
        self._lstm_packed, self._lstm_partials = None, None

    def allocate(self):
        """The concatenation buffers of a frame, twice, and the state buffers.  (The measurement maps: ``measurement_buffers``.)"""
        d, H, W = self.device, self.block.height, self.block.width
        z = lambda *s: torch.zeros(*s, device=d, dtype=torch.float32)
        if self.block.n_depth_levels != 64:
            raise ValueError("the destination-passing frame body is laid out for the network's 64 sweep planes")
        hc = 32
        direct = dict(enc_cat=[z(1, 32 + 64, H // 2, W // 2), z(1, 32 + 2 * hc, H // 4, W // 4), z(1, 32 + 4 * hc, H // 8, W // 8),
                               z(1, 32 + 8 * hc, H // 16, W // 16)],
                      dec_cat=[z(1, 16 * hc, H // 16, W // 16), z(1, 8 * hc + 1, H // 8, W // 8), z(1, 4 * hc + 1, H // 4, W // 4),
                               z(1, 2 * hc + 1, H // 2, W // 2)],
                      full_in=z(1, hc + 1 + 3, H, W), lstm_cat=z(1, 32 * hc, H // 32, W // 32),
                      estimate=z(1, 1, H // 32, W // 32), depth_store=z(1, H, W))
        # feature look-ahead (step(next_reference_image=...)): the NEXT frame's image and FPN outputs need a home while this
        # frame's encoder / decoder read their own -- a second set of the buffers the feature extraction writes and of the
        # buffer that holds the image; frames alternate between the two sets
        # and, for the deeper look-ahead (the next frame's sweep + encoder as well), of everything the encoder writes
        # ... and of the 8x10 depth estimate: a frame's splat zero-fills the OTHER set's buffer on the way (no clear launch)
        if self.sweep_mfma:      # a keyframe's half-resolution features once more, channels-last: what the feature cache keeps (written in-graph)
            direct["ref_half_nhwc"] = z(1, 32, H // 2, W // 2).contiguous(memory_format=torch.channels_last)
        keys = ("enc_cat", "dec_cat", "full_in", "lstm_cat", "estimate") + (("ref_half_nhwc",) if self.sweep_mfma else ())
        clone = lambda v: [torch.zeros_like(t) for t in v] if isinstance(v, list) else torch.zeros_like(v)
        direct["sets"] = [dict({k: direct[k] for k in keys}, index=0, meas_feat=[]),
                          dict({k: clone(direct[k]) for k in keys}, index=1, meas_feat=[])]
        self.buffers.update(direct)
        # the depth buffer IS next frame's previous depth (written once, by the last epilogue)
        self.prev_depth = direct["depth_store"].view(1, 1, H, W)
        self.h, self.c = z(1, 512, H // 32, W // 32), z(1, 512, H // 32, W // 32)

    def measurement_buffers(self, n_meas):
        """At least ``n_meas`` measurement maps in both buffer sets (channels-last where the MFMA sweep reads them)."""
        H, W = self.block.height, self.block.width
        for buffer_set in self.buffers["sets"]:
            while len(buffer_set["meas_feat"]) < n_meas:
                m = torch.zeros(1, 32, H // 2, W // 2, device=self.device, dtype=torch.float32)
                buffer_set["meas_feat"].append(m.contiguous(memory_format=torch.channels_last) if self.sweep_mfma else m)

    def repack(self):
        """After new parameters were loaded: the ConvLSTM convolution's packed copy re-packed in place (the layers' own: FusedConv2d.repack)."""
        if self._lstm_packed is not None:
            self._lstm_packed.copy_(_ops.bottleneck_conv_pack(self.lstm.lstm_cell.conv.weight.detach()))

    def _fpn_direct(self, taps, outs, half_nhwc=None):
        """FeaturePyramidNetwork.forward (dvmvs/backbone.py; torchvision's top-down pathway) with the four used outputs written
        into ``outs`` and the unused 1/32 output (fusionnet/model.py:159-164 drops it) not computed.  ``half_nhwc``: the half-resolution
        output once more, channels-last (what a later frame's MFMA sweep reads as measurement map): written by the smoothing layer's own
        epilogue (round 6; round 5: a transposing launch behind it, 5 - 16 us of every frame)."""
        fpn = self.fs.fpn
        top = fpn.inner_blocks[-1](taps[-1])
        for level in range(len(taps) - 2, -1, -1):
            top = fpn.inner_blocks[level](taps[level], residual=top, residual_mode=2)
            if level == 0 and half_nhwc is not None and isinstance(fpn.layer_blocks[0], FusedConv2d):
                fpn.layer_blocks[0](top, out=outs[0], out_nhwc=half_nhwc)
                half_nhwc = None
            else:
                fpn.layer_blocks[level](top, out=outs[level])
        if half_nhwc is not None:
            _ops.nchw_to_nhwc_into(outs[0], half_nhwc)

    def _decoder_block_direct(self, block, x, cat, depth_head, depth_input):
        """DecoderBlock.forward (dvmvs/networks.py) on the concatenation buffer ``cat`` = [up-convolution | skip | up(depth)]; the skip
        slice has already been written by the encoder's aggregator.  ``depth_head`` (the previous level's depth layer; decoder block 1 has
        none) runs as raw convolution and its bias + sigmoid are applied inside the up-sampling kernel."""
        up_channels = block.up_convolution.conv[0].weight.shape[0]
        up_conv = block.up_convolution.conv[0]
        if depth_head is not None:
            # the level's two up-samplings -- its feature map for the up-convolution, its depth head (raw convolution, bias + sigmoid on the taps) into the
            # last channel of ``cat`` -- in ONE launch (round 6; the same bits as the two)
            B, C, H, W = x.shape
            up = torch.empty((B, C, 2 * H, 2 * W), device=x.device, dtype=torch.float32)
            _ops.upsample2x_pair_into(x, up, depth_head[0](depth_input, raw=True), cat[:, -1:], depth_head[0].bias, _ops.ACTIVATIONS["sigmoid"])
            up_conv(up, out=cat[:, :up_channels])
            return block.convolution2[0](block.convolution1[0](cat))
        if isinstance(up_conv, FusedConv2d):
            up_conv.forward_upsampled(x, out=cat[:, :up_channels])
        else:
            up_conv(_ops.upsample2x(x), out=cat[:, :up_channels])
        return block.convolution2[0](block.convolution1[0](cat))

    def _lstm_bottleneck(self, x):
        """Whether the ConvLSTM convolution of input ``x`` goes through the bottleneck kernel (packs its weights the first time)."""
        if not self.bottleneck_convs:
            return False
        if self._lstm_packed is None:
            conv = self.lstm.lstm_cell.conv
            k = conv.weight.shape
            ok = conv.bias is None and tuple(k[2:]) == (3, 3) and tuple(conv.padding) == (1, 1) and tuple(conv.stride) == (1, 1) and conv.groups == 1
            splits = _ops.bottleneck_conv_splits(x.shape[0], k[0], k[1], x.shape[2], x.shape[3], 1) if ok else 0
            if splits == 0 or torch.cuda.is_current_stream_capturing():
                return False
            self._lstm_packed = _ops.bottleneck_conv_pack(conv.weight.detach())
            self._lstm_partials = torch.empty(splits * x.shape[0] * k[0] * x.shape[2] * x.shape[3], device=x.device, dtype=torch.float32)
        return True

    def _frame_body_direct(self, n_meas, has_previous, sweep_variant=0, parity=0, have=0, give=0, n_meas_next=0, next_variant=0, fork_after=-1):
        """One frame on buffer set ``parity``.  ``have``: how much of it the previous step already computed (0 nothing, 1 its reference
        features, 2 also its sweep + encoder); ``give``: how much of the NEXT frame (other buffer set) this step computes (0 / 1 / 2).
        When this frame's own share does not include a stage the next frame's share includes, the next frame's work runs on a second
        stream, concurrently with this frame's remaining stages: at batch 1 most kernels of a frame leave most of the chip idle, and
        the next frame's feature extraction, sweep and encoder depend on nothing this frame computes -- only the ConvLSTM and the
        decoder carry state (measured: tools/frame_stage_probe.py).  Same kernels on the same inputs either way: results are
        bit-identical to the one-stream frame.  ``fork_after``: where the side stream is forked off (see below)."""
        sets = self.buffers["sets"]
        cur, nxt = sets[parity], sets[1 - parity]

        def own(sweep_done=False, after_level=None):
            if have < 1:
                self._reference_features_direct(cur)
            if have < 2:
                self._sweep_encoder_direct(cur, n_meas, sweep_variant, sweep_done=sweep_done, after_level=after_level)
            self._lstm_decoder_direct(cur, has_previous)

        def ahead():
            if give >= 1:
                self._reference_features_direct(nxt)
            if give >= 2:
                self._sweep_encoder_direct(nxt, n_meas_next, next_variant)

        if give == 0:
            own()
        elif have < give:
            # (one stream: a stage's modules and scratch buffers are not run concurrently with themselves)
            own()
            ahead()
        else:
            main = torch.cuda.current_stream(self.device)
            forked = []

            def fork():
                forked.append(True)
                self.side_stream.wait_stream(main)
                with torch.cuda.stream(self.side_stream):
                    ahead()

            # WHERE the next frame's work is forked off (DVMVS_FORK_AFTER, round 6).  The frame's first kernels fill the chip on their own -- the persistent
            # sweep holds every CU's registers and LDS, the 5x5 layers of encoder level 0 run 256 workgroups -- so a side stream started next to them
            # only delays them (and waits itself); its small kernels belong next to the chain's launch-bound middle (1/8 ... 1/32 maps, ConvLSTM).
            # -1: at the start (rounds 4-5); 0: behind the sweep; k = 1 ... 4: behind encoder level k - 1.  Same kernels on the same inputs.
            level = fork_after if have == 1 else -1
            if level < 0:
                fork()
                own()
            else:
                self._sweep_direct(cur, n_meas, sweep_variant)
                if level == 0:
                    fork()
                own(sweep_done=True, after_level=(level - 1, fork) if level > 0 else None)
            if not forked:      # (a fork level the encoder does not have: the next frame would read features nobody computed)
                raise RuntimeError(f"the look-ahead was never forked off (fork level {level})")
            main.wait_stream(self.side_stream)

    def _reference_features_direct(self, buffers):
        """MnasNet taps -> FPN of the reference image of a buffer set, each used output into the front of its encoder concatenation buffer."""
        # (sweep_mfma: the copy a later frame's sweep reads as measurement map -- one 128-byte line per cell -- is made here, inside the frame graph, so
        # that the feature cache's per-keyframe copy stays a plain device copy on the host's side)
        self._fpn_direct(self.fe(buffers["full_in"][:, 33:36]), [c[:, :32] for c in buffers["enc_cat"]],
                         half_nhwc=buffers["ref_half_nhwc"] if self.sweep_mfma else None)

    def _sweep_direct(self, buffers, n_meas, sweep_variant=0):
        """Plane sweep of the frame whose features are in ``buffers``, into the cost-volume slice of its first encoder concatenation buffer."""
        block, s = self.block, self.block.views
        enc_cat = buffers["enc_cat"]
        Hm, kt = block.sweep_views(n_meas, buffers["index"])
        if block.pose_algebra == "exact":
            Hm, kt = _ops.sweep_matrices(s["pose"], s["meas_pose"][:n_meas], s["half_K"])
        _ops.cost_volume_into(enc_cat[0][:, :32], buffers["meas_feat"][:n_meas], Hm, kt, block.min_depth, block.max_depth, enc_cat[0][:, 32:], sweep_variant,
                              block.sweep_items(buffers["index"]))

    def _sweep_encoder_direct(self, buffers, n_meas, sweep_variant=0, sweep_done=False, after_level=None):
        """Plane sweep + cost-volume encoder of the frame whose features are in ``buffers``: reads that set's measurement features and
        sweep parameters, writes its skip connections (into the decoder's concatenation buffers) and its bottleneck map.  Depends on
        nothing the PREVIOUS frame computes -- no recurrent state, no previous depth -- which is what lets it run a frame ahead."""
        enc_cat, dec_cat = buffers["enc_cat"], buffers["dec_cat"]
        if not sweep_done:
            self._sweep_direct(buffers, n_meas, sweep_variant)
        # encoder: aggregator output = skip connection, written where the decoder will read it
        enc = self.enc
        for level in range(4):
            skip_channels = getattr(enc, f"aggregator{level}")[0].weight.shape[0]
            cat = dec_cat[3 - level]
            up_channels = cat.shape[1] - skip_channels - (1 if level < 3 else 0)
            skip = getattr(enc, f"aggregator{level}")[0](enc_cat[level], out=cat[:, up_channels:up_channels + skip_channels])
            block = getattr(enc, f"encoder_block{level}")
            x = block.standard_convolution.conv1[0](block.down_convolution.down_conv[0](skip))
            if level < 3:
                block.standard_convolution.conv2[0](x, out=enc_cat[level + 1][:, 32:])
            else:
                block.standard_convolution.conv2[0](x, out=buffers["lstm_cat"][:, :512])      # (pairnet: the buffer is just the bottleneck's home)
            if after_level is not None and after_level[0] == level:
                after_level[1]()      # (the look-ahead fork: _frame_body_direct)

    def _state_warp_direct(self, buffers, has_previous):
        """Re-projection of the previous depth into the frame's 8x10 estimate and the hidden state warped with it into the ConvLSTM's input
        (convlstm.py:27-41, utils.py:110-154).  Reads the previous frame's depth and state only -- nothing of this frame's sweep or encoder."""
        s = self.block.views
        lstm_cat = buffers["lstm_cat"]
        if has_previous:
            exact = self.block.pose_algebra == "exact"
            reproject_T = _ops.relative_pose(s["pose"], s["prev_pose"]) if exact else s["reproject_T"]
            lstm_T = _ops.relative_pose(s["prev_pose"], s["pose"]) if exact else s["lstm_T"]
            # re-projection of the previous depth straight into this buffer set's 8x10 estimate (one launch: it also zero-fills the
            # other set's estimate for the next frame), then the hidden-state warp
            other = self.buffers["sets"][1 - buffers["index"]]["estimate"]
            _ops.depth_reproject_estimate_into(reproject_T, self.prev_depth, s["full_K"], s["half_K"], buffers["estimate"], other, 16)
            _ops.hidden_warp_into(self.h, buffers["estimate"], lstm_T, s["lstm_K"], True, lstm_cat[:, 512:])
        else:
            lstm_cat[:, 512:].copy_(self.h)      # first frame of a sequence: the (zero) state as it is, no warp (convlstm.py:29)

    def _lstm_decoder_direct(self, buffers, has_previous):
        """Re-projection of the previous depth, ConvLSTM and decoder of the frame whose encoder outputs are in ``buffers``: the part of a
        frame that carries the recurrent state."""
        dec, dec_cat, lstm_cat = self.dec, buffers["dec_cat"], buffers["lstm_cat"]
        bottom = lstm_cat[:, :512]
        if self.is_fusionnet:
            cell = self.lstm.lstm_cell
            self._state_warp_direct(buffers, has_previous)
            if self._lstm_bottleneck(lstm_cat):
                # the 1024 -> 2048-channel convolution as K-split partial sums (75 MB of weights streamed once through the MFMA
                # pipe); the gates kernel adds the partial sums itself, in ascending order (one wave per LayerNorm row): no reduction launch
                splits = _ops.bottleneck_conv_into(lstm_cat, self._lstm_packed, cell.conv.weight.shape[0], 1, self._lstm_partials)
                _ops.lstm_gates_partials_into(self._lstm_partials, splits, self.c, self.h)
            else:
                combined = cell.conv(lstm_cat)
                if not combined.is_contiguous():       # channels-last convolution (lstm_channels_last): back to the gates' NCHW rows
                    combined = combined.contiguous()
                _ops.lstm_gates_into(combined, self.c, self.h)
            bottom = self.h
        d1 = self._decoder_block_direct(dec.decoder_block1, bottom, dec_cat[0], None, None)
        d2 = self._decoder_block_direct(dec.decoder_block2, d1, dec_cat[1], dec.depth_layer_one_sixteen, d1)
        d3 = self._decoder_block_direct(dec.decoder_block3, d2, dec_cat[2], dec.depth_layer_one_eight, d2)
        d4 = self._decoder_block_direct(dec.decoder_block4, d3, dec_cat[3], dec.depth_layer_quarter, d3)
        full_in = buffers["full_in"]
        _ops.upsample2x_pair_into(d4, full_in[:, :32], dec.depth_layer_half[0](d4, raw=True), full_in[:, 32:33], dec.depth_layer_half[0].bias,
                                  _ops.ACTIVATIONS["sigmoid"])
        refined = dec.refine[1][0](dec.refine[0][0](full_in))
        # last convolution: bias + sigmoid + depth mapping (model.py:231-232) in one epilogue, into the depth / previous-depth buffer
        dec.depth_layer_full[0](refined, out=self.prev_depth, activation=_ops.ACTIVATION_SIGMOID_TO_DEPTH,
                                p0=dec.inverse_depth_multiplier, p1=dec.inverse_depth_base)
