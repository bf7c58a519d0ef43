// switches.h -- the run-time GSDR_* switches as one value.  No HIP here: the launch rules that read them (ddc_plan.h,
// pfb_plan.h) are asked by host_logic.cpp too, which is built alone by a host compiler.
#ifndef GSDR_SWITCHES_H
#define GSDR_SWITCHES_H

namespace gsdr {

// The run-time GSDR_* switches (A/B runs and the tests; INTEGRATION.md, "Run-time knobs"), read from the environment
// by read_switches() when a handle is created and kept by it: nothing reads the environment after that.  Each field
// holds what the variable selects, with the default when it is unset or empty; -1 / 0 marked "unset" leave the
// default to the one place that uses the field.
struct Switches {
    bool ddc_mfma = true;       // GSDR_DDC_MFMA, 1: matrix-core DDC where its shape rules hold; 0: ddc_flat_kernel (F <= 4)
    bool ddc_few = true;        // GSDR_DDC_FEW, 1: ddc_few_kernel for a handful of tones at decim >= 512; 0: never
    bool ddc_pipe = true;       // GSDR_DDC_PIPE, 1: ddc_flat_kernel where it may run; 0: the generic ddc_kernel
    int ddc_k = -1;             // GSDR_DDC_K, -1 unset: phasor-table length 16 / the flat kernel's sub-block by shape
    int ddc_waves = 0;          // GSDR_DDC_WAVES_PER_SIMD, 0 unset: resident waves per SIMD, 6 (flat kernel) or 4; <= 0: 4
    int ddc_nch = 0;            // GSDR_DDC_NCH, 0: chunks per DDC launch by the grid rule; > 0: that many
    unsigned ddc_lds = 0;       // GSDR_DDC_LDS, 0: dummy LDS bytes per DDC workgroup (occupancy cap)
    int ddc_prefetch = 1;       // GSDR_DDC_PREFETCH, 1: ddc_flat_kernel prefetches the IQ stream into L2; 0: not
    bool ddc_autotune = true;   // GSDR_DDC_AUTOTUNE, 1: ddc_flat_kernel's grid timed at create; 0: ratio 1.3
    int mfma_asm = 4;           // GSDR_MFMA_ASM, 4: ring16 loop; 5: its 8-wave form; 2: round 1's ring; else the C++ kernel
    int mfma_tt = 1;            // GSDR_MFMA_TT, 1: C++ kernel tone tiles per wave (1 or 2)
    int mfma_pk = 32;           // GSDR_MFMA_PK, 32: C++ kernel phasor block (16 or 32)
    int mfma_w = 4;             // GSDR_MFMA_W, 4: C++ kernel waves per workgroup (2 or 4)
    int mfma_rt = 0;            // GSDR_MFMA_RT, 0: ring kernel row tiles per workgroup chosen per launch; 1, 2: forced
    bool mfma_w8 = true;        // GSDR_MFMA_W8, 1: in-order launches that fit run the 8-wave ring16 kernel; 0: never
    int mfma_prec = -1;         // GSDR_MFMA_PREC, -1: pre-converted operands per launch; 1: always; else never
    int mfma_3m = -1;           // GSDR_MFMA_3M, -1 unset: three real products per complex multiply on handles with pre-converted
                                // images and a window of kMac3MinBlocks blocks or more; 1: wherever there are images; else never
    int mfma_3m_rot = -1;       // GSDR_MFMA_3M_ROT, -1 unset: three-product handles with a window of kRot2MinBlocks blocks or more
                                // rotate their partial sums once per pair of blocks; 2: every three-product handle; else per block
    int mfma_fold = -1;         // GSDR_MFMA_FOLD, -1 unset: handles that rotate per pair and have a window of kFoldMinBlocks blocks or
                                // more fold each 64-sample span about its centre (48 MFMAs per span for 72); 1: every such handle; else never
    int mfma_fold_products = -1;    // GSDR_MFMA_FOLD_PRODUCTS, -1 unset: a folded handle sums the plain four products straight into Re and Im
                                // (ddc_mfma_ring16p4f_kernel); 3: Gauss's three (ddc_mfma_ring16p3f_kernel); 4: the four
    int mfma_wave_tones = -1;   // GSDR_MFMA_WAVE_TONES, -1 unset: a handle that sums the plain four products takes the loop with wave tiles of
                                // 16 rows x 64 tones (ddc_mfma_ring16p4fw_kernel) when that launches no more waves; 64: every such handle; 32: never
    int mfma_span = -1;         // GSDR_MFMA_SPAN, -1 unset: a handle that took the wide tile by its own rule (GSDR_MFMA_WAVE_TONES unset) and has a
                                // window of kSpan128MinBlocks blocks or more rotates once per 128 samples (ddc_mfma_ring16p4fw2_kernel); 128: every
                                // handle on the wide tile; 64 (or anything else): never
    int mfma_timing = 0;        // GSDR_MFMA_TIMING, 0: timing-only modes 1 - 3 (builds with -DGSDR_TIMING_BUILD only)
    bool noise_fft = true;      // GSDR_NOISE_FFT, 1: NOISE through the polyphase filter + FFT; 0: every bin a DDC tone
    bool tones_fft = true;      // GSDR_TONES_FFT, 1: TONES through filter + FFT + bin selection; 0: every bin a DDC tone
    bool pfb_lds = true;        // GSDR_PFB_LDS, 1: TONES / NOISE inside the LDS where the frame fits; 0: never
    int pfb_bluestein = -1;     // GSDR_PFB_BLUESTEIN, -1 unset: Bluestein in the LDS for primes above 127 only; 1: also others; 0: never
    int pfb_cu = -1;            // GSDR_PFB_CU, -1: pfb_cu_kernel by shape; 0: never; 1: forced (other values: forced, fill rule kept)
    bool pfb_direct = true;     // GSDR_PFB_DIRECT, 1: pfb_cu_kernel filters straight out of global memory; 0: through the LDS
    int pfb_col = -1;           // GSDR_PFB_COL, -1: staged filter column-wise by shape; 1: column-wise; 0: point-wise
    int pfb_cu_nt = 0;          // GSDR_PFB_CU_NT, 0: pfb_cu_kernel workgroup by shape; 512: two per unit; else 1024
    bool pfb_teams = true;      // GSDR_PFB_TEAMS, 1: the frames of a run go through their stages in teams; 0: in step
    bool pfb_radix8 = true;     // GSDR_PFB_RADIX8, 1: radix 8 / 6 / 10 stages in the LDS; 0: radix 4 / 2
    int pfb_fr = 0;             // GSDR_PFB_FR, 0: pfb_lds_kernel frames per workgroup by shape; > 0: that many
    int pfb_wide = -1;          // GSDR_PFB_WIDE, -1: pfb_lds_kernel 512 threads from 2048 points; 1: always; 0: 256
    int mix_few = 32;           // GSDR_MIX_FEW, 32: up to how many tones mix_few_kernel runs (decim 0); 0: never
    bool chirp_split = true;    // GSDR_CHIRP_SPLIT, 1: long lock-in points summed by several waves; 0: a wave per point
    bool pipe_queues = true;    // GSDR_PIPE_QUEUES, 1: compute streams with a CU mask (a queue each); 0: plain streams
    bool pipe_overlap = true;   // GSDR_PIPE_OVERLAP, 1: consecutive submitted DIRECT buffers on rotating streams; 0: one
    int pipe_streams = 3;       // GSDR_PIPE_STREAMS, 3: compute streams the overlap rotates over (1 ... 3, else 3)
};
Switches read_switches();

}  // namespace gsdr

#endif
