// aes_core_test.cc -- the entry points of csrc/kernels/aes_core.h on the host
// (HostLookup tables, ArrayRK round keys; no GPU library):
//   * encrypt against FIPS-197 Appendix C.1;
//   * mmo_hash against known answers given on the command line as triples of
//     32-digit hex uint128 values (key, input, expected hash) -- the caller
//     reads them from tests/golden/aes_kat.json;
//   * encrypt2, encryptN<1..4>, encryptAB<2,2> (two different keys) against
//     encrypt, block by block, on 64 pseudo-random blocks;
//   * mmo_hash2, mmo_hashN<1..4>, mmo_hashAB<2,2> likewise against mmo_hash.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "aes_core.h"

using dpf_aes::ArrayRK;
using dpf_aes::Block4;
using dpf_aes::HostLookup;

namespace {

int failures = 0;

void check(bool ok, const char* what, int i) {
  if (!ok) {
    ++failures;
    printf("FAIL %s [%d]\n", what, i);
  }
}

bool eq(Block4 a, Block4 b) { return a.w0 == b.w0 && a.w1 == b.w1 && a.w2 == b.w2 && a.w3 == b.w3; }

// 16 bytes, in memory order, as the block's four little-endian columns.
Block4 from_bytes(const uint8_t b[16]) {
  uint32_t w[4];
  for (int i = 0; i < 4; ++i)
    w[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
           ((uint32_t)b[4 * i + 3] << 24);
  return Block4{w[0], w[1], w[2], w[3]};
}

// A uint128 written as 32 hex digits (most significant first) -> its
// little-endian memory image.
bool parse_u128(const char* hex, uint8_t out[16]) {
  if (strlen(hex) != 32) return false;
  for (int i = 0; i < 16; ++i) {
    unsigned v;
    if (sscanf(hex + 2 * i, "%2x", &v) != 1) return false;
    out[15 - i] = (uint8_t)v;
  }
  return true;
}

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}
Block4 rnd_block() { return Block4{rnd(), rnd(), rnd(), rnd()}; }

template <int N>
void check_n(const HostLookup& lk, ArrayRK key, const Block4* x, int base) {
  const Block4* in = x + base;
  ArrayRK rk[N];
  Block4 e[N], h[N];
  for (int i = 0; i < N; ++i) {
    rk[i] = key;
    e[i] = h[i] = in[i];
  }
  dpf_aes::encryptN<N>(e, lk, rk);
  dpf_aes::mmo_hashN<N>(h, lk, rk);
  for (int i = 0; i < N; ++i) {
    check(eq(e[i], dpf_aes::encrypt(in[i], lk, key)), "encryptN", base + i);
    check(eq(h[i], dpf_aes::mmo_hash(in[i], lk, key)), "mmo_hashN", base + i);
  }
}

}  // namespace

int main(int argc, char** argv) {
  const HostLookup lk;

  // FIPS-197 Appendix C.1.
  {
    uint8_t key[16], pt[16];
    for (int i = 0; i < 16; ++i) {
      key[i] = (uint8_t)i;
      pt[i] = (uint8_t)(0x11 * i);
    }
    const uint8_t ct[16] = {0x69, 0xc4, 0xe0, 0xd8, 0x6a, 0x7b, 0x04, 0x30,
                            0xd8, 0xcd, 0xb7, 0x80, 0x70, 0xb4, 0xc5, 0x5a};
    uint32_t rk[44];
    dpf_aes::expand_key(key, rk);
    check(eq(dpf_aes::encrypt(from_bytes(pt), lk, ArrayRK{rk}), from_bytes(ct)), "fips197 C.1", 0);
  }

  // Known answers of the MMO hash.
  int kat = 0;
  for (int a = 1; a + 2 < argc; a += 3, ++kat) {
    uint8_t key[16], in[16], out[16];
    if (!parse_u128(argv[a], key) || !parse_u128(argv[a + 1], in) || !parse_u128(argv[a + 2], out)) {
      printf("bad known-answer argument %d\n", a);
      return 2;
    }
    uint32_t rk[44];
    dpf_aes::expand_key(key, rk);
    check(eq(dpf_aes::mmo_hash(from_bytes(in), lk, ArrayRK{rk}), from_bytes(out)), "mmo_hash kat", kat);
  }

  // The interleaved forms against the single-block ones, two different keys.
  constexpr int kBlocks = 64;
  uint8_t ka[16], kb[16];
  for (int i = 0; i < 16; ++i) {
    ka[i] = (uint8_t)rnd();
    kb[i] = (uint8_t)rnd();
  }
  uint32_t rka[44], rkb[44];
  dpf_aes::expand_key(ka, rka);
  dpf_aes::expand_key(kb, rkb);
  const ArrayRK A{rka}, B{rkb};
  Block4 x[kBlocks];
  for (int i = 0; i < kBlocks; ++i) x[i] = rnd_block();

  for (int i = 0; i < kBlocks; i += 2) {
    Block4 ea = x[i], eb = x[i + 1], ha = x[i], hb = x[i + 1];
    dpf_aes::encrypt2(ea, eb, lk, A, B);
    dpf_aes::mmo_hash2(ha, hb, lk, A, B);
    check(eq(ea, dpf_aes::encrypt(x[i], lk, A)), "encrypt2 a", i);
    check(eq(eb, dpf_aes::encrypt(x[i + 1], lk, B)), "encrypt2 b", i + 1);
    check(eq(ha, dpf_aes::mmo_hash(x[i], lk, A)), "mmo_hash2 a", i);
    check(eq(hb, dpf_aes::mmo_hash(x[i + 1], lk, B)), "mmo_hash2 b", i + 1);
  }
  for (int i = 0; i < kBlocks; i += 1) check_n<1>(lk, i & 1 ? B : A, x, i);
  for (int i = 0; i < kBlocks; i += 2) check_n<2>(lk, i & 2 ? B : A, x, i);
  for (int i = 0; i + 3 <= kBlocks; i += 3) check_n<3>(lk, i & 1 ? B : A, x, i);
  check_n<1>(lk, B, x, kBlocks - 1);  // 64 = 21 * 3 + 1
  for (int i = 0; i < kBlocks; i += 4) check_n<4>(lk, i & 4 ? B : A, x, i);
  for (int i = 0; i < kBlocks; i += 4) {
    const ArrayRK ra[2] = {A, A}, rb[2] = {B, B};
    Block4 e[4], h[4];
    for (int j = 0; j < 4; ++j) e[j] = h[j] = x[i + j];
    dpf_aes::encryptAB<2, 2>(e, lk, ra, rb);
    dpf_aes::mmo_hashAB<2, 2>(h, lk, ra, rb);
    for (int j = 0; j < 4; ++j) {
      check(eq(e[j], dpf_aes::encrypt(x[i + j], lk, j < 2 ? A : B)), "encryptAB<2,2>", i + j);
      check(eq(h[j], dpf_aes::mmo_hash(x[i + j], lk, j < 2 ? A : B)), "mmo_hashAB<2,2>", i + j);
    }
  }
  // The two keys must tell apart: a form that ignored its second key would
  // otherwise pass.
  check(!eq(dpf_aes::encrypt(x[0], lk, A), dpf_aes::encrypt(x[0], lk, B)), "keys differ", 0);

  printf("aes_core: %d known answers, %d blocks, %d failures\n", kat, kBlocks, failures);
  return failures ? 1 : 0;
}
