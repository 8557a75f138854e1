// aux_kernels.inc -- the small kernels the host API launches around the frame engines: scene build (primitive gather,
// conservative 48-B nodes, filter fields) and the frame assembly of the several-devices entry.  Included from api.inc,
// inside its anonymous namespace.
// Scene upload: primitives arrive in flatten order (packed and copied while the BVH is being built) and are put into
// slot order here -- one thread per 16 B of a 256-B shading record, the first nine of a primitive also move one float
// of its triangle.
__global__ void k_gather_prims(const uint32_t* __restrict__ order, const float* __restrict__ tris_flat, const uint4* __restrict__ ext_flat,
                               float* __restrict__ tris, uint4* __restrict__ ext, uint32_t count) {
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t slot = gid >> 4, part = gid & 15u;
  if (slot >= count) return;
  const uint32_t src = order[slot];
  ext[(size_t)slot * 16 + part] = ext_flat[(size_t)src * 16 + part];
  // the slot's 48-B primitive record: nine floats of the triangle, then the filter fields (k_fill_tri_filter) -- until then
  // rank = slot (ties to the lower slot: RAYCA_BUILDER_REFERENCE) and leaf 0
  if (part < kTriFloats) {
    float v = 0.0f;
    if (part < 9) v = tris_flat[(size_t)src * 9 + part];
    else if (part == 9) v = __uint_as_float(slot);
    tris[(size_t)slot * kTriFloats + part] = v;
  }
}

// RAYCA_NODE_CH: every box of the binary nodes as centre + half extent, containing the box it is made from: the centre is rounded
// to nearest, the half extent takes the centre's rounding error and is rounded up.  RAYCA_NODE_CH48 (trace_core.inc): 48-B records,
// the child references in the low halves of the x and y half extents, which are rounded up to 8 mantissa bits first.
struct ChNode48 { float q[12]; };
__device__ __forceinline__ float ch_carry(float h, uint32_t ref16, bool one_more = false) {
  uint32_t b = __float_as_uint(h);                        // h >= 0
  b = (b + 0xFFFFu) & 0xFFFF0000u;                        // up to a multiple of 2^16 ulps
  if (one_more) b += 0x10000u;
  if (b > 0x7F7F0000u) b = 0x7F7F0000u;                   // (never an infinity: with a reference below it that would be a NaN)
  return __uint_as_float(b | ref16);
}
// a child reference as this array's records hold it: an inner one is the child's byte offset (kChRefScale)
__host__ __device__ __forceinline__ uint32_t ch_ref(uint32_t ref) { return ((ref & kLeafFlag) || ref == kNoChild || ref == kTerminated) ? ref : ref * kChRefScale; }
__global__ void k_make_ch_nodes(const DevNode* __restrict__ nodes, void* __restrict__ out, uint32_t count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  DevNode d = nodes[i];
  // A link of the chain that splits a leaf above 64 primitives: two identical boxes, 64 primitives on the left, the rest of the
  // chain on the right.  Its stack need (one entry) holds only while the left child is entered first, that is while the left box
  // is entered no later than the right one -- and below, the references make the two x and y half extents differ.  The left
  // ones get one step of 2^16 ulps more, so that they are the larger ones whatever the references are (a front-to-back
  // search that entered the right child first kept one leaf pending per link and ran past its stack).
  bool chain_link = (d.left & kLeafFlag) && ((d.left >> 25) & 63u) == 63u && !(d.right & kLeafFlag) && d.right != kNoChild;
  for (int k = 0; k < 6; ++k) chain_link = chain_link && __float_as_uint(d.q[k]) == __float_as_uint(d.q[6 + k]);
  for (int b = 0; b < 2; ++b) {
    float* q = d.q + 6 * b;
    for (int a = 0; a < 3; ++a) {
      const double lo = q[a], hi = q[3 + a];
      const double cd = 0.5 * (lo + hi);
      const float c = (float)cd;
      const double hd = 0.5 * (hi - lo) + fabs((double)c - cd);
      float h = (float)hd;
      if ((double)h < hd) h = nextafterf(h, INFINITY);
      q[a] = c;
      q[3 + a] = h;
    }
  }
#if RAYCA_NODE_CH48
  ChNode48 o;
  for (int k = 0; k < 12; ++k) o.q[k] = d.q[k];
  const uint32_t l = ch_ref(d.left), r = ch_ref(d.right);
  o.q[3] = ch_carry(d.q[3], l & 0xFFFFu, chain_link);
  o.q[4] = ch_carry(d.q[4], l >> 16, chain_link);
  o.q[9] = ch_carry(d.q[9], r & 0xFFFFu);
  o.q[10] = ch_carry(d.q[10], r >> 16);
  static_cast<ChNode48*>(out)[i] = o;
#else
  static_cast<DevNode*>(out)[i] = d;
#endif
}

// RAYCA_BUILDER_SAH: the filter fields of every primitive record -- its rank in the reference's order and its reference leaf
__global__ void k_fill_tri_filter(float* __restrict__ tris, const uint32_t* __restrict__ tie_rank, const uint32_t* __restrict__ ref_leaf_of, uint32_t count) {
  const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= count) return;
  float* t = tris + (size_t)slot * kTriFloats;
  t[9] = __uint_as_float(tie_rank ? tie_rank[slot] : slot);
  t[10] = __uint_as_float(ref_leaf_of ? ref_leaf_of[slot] : 0u);
}

// frame row y <- gathered row: band b = y / band lives with part b % parts at position (b / parts) * band + y % band
__global__ __launch_bounds__(256) void k_deinterleave(const uint32_t* gathered, uint32_t* frame, uint32_t width, uint32_t height, uint32_t parts,
                                                      uint32_t band, uint32_t max_rows) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= width * height) return;
  const uint32_t y = i / width, x = i - y * width;
  const uint32_t b = y / band, part = b % parts, pos = (b / parts) * band + (y % band);
  frame[i] = gathered[((size_t)part * max_rows + pos) * width + x];
}
