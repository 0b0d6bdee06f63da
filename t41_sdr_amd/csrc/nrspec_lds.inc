// t41_sdr_amd/csrc/nrspec_lds.inc -- the LDS of nrspec_kernel and nrspec_map_kernel (nr_kernels.hip), included at the top of
// the kernel's body.  KLDS, a constant of the including kernel, is the kind the memories are laid out for: the kernel's own
// KIND in nrspec_kernel<KIND>, 1 in nrspec_map_kernel, whose workgroups run either kind (Kim1_NR()'s is the larger).
  // One region serves, one after the other within a frame, as the FFT's exchange buffer, the spectrum for the partner
  // access, the two weighted spectra and the two output frames: a workgroup is ONE wave, whose LDS operations execute
  // in program order, and each tenant is dead (in registers) before the next one is written.  With the per-bin
  // memories that leaves the spectral function under 10 KiB, i.e. 16 workgroups per CU: the whole 4096-channel batch
  // resident in one round instead of two.
  __shared__ __attribute__((aligned(16))) float U[8 * kFftRow * 2];
  static_assert(8 * kFftRow * 2 >= 520 && 8 * kFftRow * 2 >= 512, "tenants of the shared region");
  float *xbuf = U;                               // FFT exchange
  cf *Zs = reinterpret_cast<cf *>(U);            // [257] the 256-point spectrum of frame 0 + j frame 1 (partner access), [256] = [0]
  cf *W0 = reinterpret_cast<cf *>(U), *W1 = reinterpret_cast<cf *>(U + 260);  // [129] each: weighted, conjugate-symmetrised spectra, bins 0..128
  float *Y0 = U, *Y1 = U + 256;                  // [256] each
  __shared__ float S[384];          // NR_last_sample_buffer_L | the block's 256 samples
  __shared__ float Gb[130];         // gains with one pad either side: Gb[1 + i]
  constexpr int KW = (KLDS == 1) ? 128 : 1;  // (Kim1_NR()'s memories only)
  __shared__ float Xs[KLDS == 1 ? 3 : 1][KW], Es[KLDS == 1 ? 15 : 1][KW];  // Kim1_NR()'s frame histories
  __shared__ float Gts1[KW], Gts0[KW];
  __shared__ float GstP[8 + 128 + 8];  // (padded: the smoothing windows of the edge bins reach 8 below / 4 above)
  float *Gst = GstP + 8;
  __shared__ float Lout[128], Nest[128], Pslp[128], Xt[128], Hk[128];
